"""GPU parity tests of the fused fast path (gaussian_splatting_amd.fused): stage-wise bit-exact
against the CPU oracle, end-to-end against the reference-shaped path and the golden fixtures."""
import numpy as np
import pytest
import torch

from gaussian_splatting_amd import fused
from gaussian_splatting_amd.splat_py.rasterize import rasterize as rasterize_mirror
from gaussian_splatting_amd.synthetic import make_grad_image, make_scene

from .helpers import load, oracle_stages, oracle_vjp, report, scaled_err, scene6, scene_from_fixture, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_TOL = 1e-4
E2E_GRAD_TOL = 1e-4   # whole chain vs the reference's host pipeline, frames without a flipped threshold decision
PARAMS = ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")


def oracle():
    from oracle import gs_oracle
    gs_oracle.set_modes(0, 0)
    gs_oracle.set_sh_band1_mode(0)
    return gs_oracle


def cpu_expected_stages(g, cam, T, near, far, pad, mh):
    """the fused forward restated on the CPU with the oracle's kernels (tests/helpers.py: oracle_stages, fp32); the
    world->camera transform is written as the same explicit fp32 expression the kernel uses"""
    return oracle_stages(g, cam, T, near, far, pad, torch.float32, mh=mh)


@pytest.mark.parametrize("N,W,H,deg,seed", [(1000, 256, 256, 0, 0), (20000, 640, 472, 3, 1), (5000, 200, 120, 1, 2),
                                            (5000, 200, 120, 2, 3)])
def test_fused_forward_stages_bit_exact(N, W, H, deg, seed):
    orc = oracle()
    g, cam, T = make_scene(N, W, H, deg, seed=seed)
    T = T.clone()
    T[:3, :3] = torch.tensor([[0.9999, 0.0089, 0.0073], [-0.0106, 0.9568, 0.2905], [-0.0044, -0.2906, 0.9568]])
    T[:3, 3] = torch.tensor([0.05, -0.1, 0.3])
    near, far, pad, mh = 2.0, 25.0, 20, 3.0
    exp = cpu_expected_stages(g, cam, T, near, far, pad, mh)
    gd, camd, Td = make_scene(N, W, H, deg, seed=seed, device=DEV)
    bg = torch.full((3,), 0.5)
    image, mask, uv, aux = fused.rasterize(gd, T.to(DEV), camd, near, far, pad, mh, True, bg.to(DEV), return_aux=True)
    V = exp["V"]
    assert 0 < V < N
    assert torch.equal(mask.cpu(), exp["culled"])
    assert torch.equal(uv.cpu(), exp["uv"])
    assert torch.equal(aux["xyz_camera_frame"].cpu(), exp["xyz_c"])
    assert torch.equal(aux["conic"].cpu(), exp["conic"])
    assert torch.equal(aux["opacity"].cpu(), exp["opacity"])
    assert torch.equal(aux["vis_idx"].cpu().long(), torch.nonzero(~exp["culled"]).flatten())
    assert torch.equal(aux["tile_ranges"].cpu(), exp["ranges"])
    assert torch.equal(aux["sorted_gaussians"].cpu(), exp["sorted"])
    # colour: the camera centre is formed in fp64 on both sides but by different algorithms
    assert (aux["rgb"].cpu() - exp["rgb"]).abs().max() < 2e-6
    # render: the oracle on the kernel's own per-splat inputs -> bit-identical image
    img = torch.zeros(H, W, 3)
    nsp = torch.zeros(H, W, dtype=torch.int32)
    fw = torch.zeros(H, W)
    orc.render_tiles_cuda(exp["uv"], exp["opacity"], aux["rgb"].cpu().contiguous(), exp["conic"], torch.zeros(1, 1, 1),
                          exp["ranges"], exp["sorted"], bg, nsp, fw, img)
    assert torch.equal(image.cpu(), img)


@pytest.mark.parametrize("N,W,H,deg,seed,bgval", [(1000, 256, 256, 0, 0, 0.0), (20000, 640, 472, 3, 1, 0.5),
                                                   (150000, 3840, 2160, 1, 7, 0.0)])
def test_fused_matches_reference_shaped_path(hip_backend, N, W, H, deg, seed, bgval):
    """same frame through the six-node path and through the fused path: forward within the
    tolerance of an ulp-level difference in the world->camera transform, gradients 1e-4.  The third case is a 4K
    frame: 32 400 tiles, more than an LDS histogram holds -- the fused frame bins with the global-counter kernels"""
    bg = torch.full((3,), bgval, device=DEV)
    gi = make_grad_image(W, H, seed=seed + 9, device=DEV)
    outs = []
    for fn in (rasterize_mirror, fused.rasterize):
        g, cam, T = make_scene(N, W, H, deg, seed=seed, device=DEV)
        for k in PARAMS:
            if getattr(g, k) is not None:
                getattr(g, k).requires_grad_(True)
        img, mask, uv = fn(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg)
        uv.retain_grad()
        img.backward(gi)
        outs.append((img.detach(), mask, uv.detach(), uv.grad, {k: getattr(g, k).grad for k in PARAMS
                                                                  if getattr(g, k) is not None}))
    (i0, m0, u0, gu0, p0), (i1, m1, u1, gu1, p1) = outs
    assert torch.equal(m0, m1)
    assert (u0 - u1).abs().max() < 1e-3
    diff = (i0 - i1).abs().amax(dim=2)
    assert (diff > 1e-5).float().mean() < 2e-3 and diff.max() < 5e-3
    errs = {k: scaled_err(p1[k], p0[k]) for k in p0}
    errs["uv"] = scaled_err(gu1, gu0)
    report(f"fused_vs_reference_shaped[{N}-deg{deg}]", image_max_diff=diff.max().item(),
           pixels_over_1e5=(diff > 1e-5).float().mean().item(), grad_scaled_err=max(errs.values()))
    for k in p0:
        assert p1[k].shape == p0[k].shape
    # a flipped alpha >= 1/255 decision would cost up to 5e-3 (test_end_to_end_difference_is_flipped_
    # threshold_decisions); none flips on these frames and the whole chain agrees to 1e-4
    assert max(errs.values()) < E2E_GRAD_TOL, errs


@pytest.mark.parametrize("N,W,H,deg,seed,bgval", [(20000, 640, 472, 3, 1, 0.5), (6000, 328, 200, 1, 4, 0.0),
                                                   (6000, 328, 200, 2, 5, 0.25)])
def test_fused_per_pixel_sh_matches_reference_shaped_path(hip_backend, N, W, H, deg, seed, bgval):
    """use_sh_precompute=False (rasterize.py:100-110; render.cu:283-333, render_backward.cu:422-488): the fused
    frame's per-Gaussian stage / binning / sort with the N_SH = 4, 9, 16 render kernels against the six-node
    path of the same colour mode -- same tolerances as the precompute mode's comparison above"""
    bg = torch.full((3,), bgval, device=DEV)
    gi = make_grad_image(W, H, seed=seed + 9, device=DEV)
    outs = []
    for fn in (rasterize_mirror, fused.rasterize):
        g, cam, T = make_scene(N, W, H, deg, seed=seed, device=DEV)
        for k in PARAMS:
            if getattr(g, k) is not None:
                getattr(g, k).requires_grad_(True)
        img, mask, uv = fn(g, T, cam, 0.3, 500.0, 100, 3.0, False, bg)
        uv.retain_grad()
        img.backward(gi)
        outs.append((img.detach(), mask, uv.detach(), uv.grad, {k: getattr(g, k).grad for k in PARAMS
                                                                  if getattr(g, k) is not None}))
    (i0, m0, u0, gu0, p0), (i1, m1, u1, gu1, p1) = outs
    assert torch.equal(m0, m1)
    assert (u0 - u1).abs().max() < 1e-3
    diff = (i0 - i1).abs().amax(dim=2)
    assert (diff > 1e-5).float().mean() < 2e-3 and diff.max() < 5e-3
    errs = {k: scaled_err(p1[k], p0[k]) for k in p0}
    errs["uv"] = scaled_err(gu1, gu0)
    report(f"fused_per_pixel_sh_vs_reference_shaped[{N}-deg{deg}]", image_max_diff=diff.max().item(),
           grad_scaled_err=max(errs.values()))
    for k in p0:
        assert p1[k].shape == p0[k].shape
    assert p1["sh"].abs().max() > 0 and p1["rgb"].abs().max() > 0
    assert max(errs.values()) < E2E_GRAD_TOL, errs


def test_fused_render_depth_matches_reference_shaped_path(hip_backend):
    """depth.py:17-88 through the fused stages against the six-node mirror: the same depth wherever the two
    per-Gaussian stages (ulp-level different world->camera transform) make the same threshold decisions"""
    from gaussian_splatting_amd.splat_py.depth import render_depth as mirror_depth
    N, W, H = 20000, 640, 472
    g, cam, T = make_scene(N, W, H, 0, seed=3, device=DEV)
    ref = mirror_depth(g, 0.5, T, cam, 0.3, 100, 3.0)
    got = fused.render_depth(g, 0.5, T, cam, 0.3, 100, 3.0)
    assert got.shape == ref.shape == (H, W, 1) and got.dtype == torch.float32
    assert (ref > 0).float().mean() > 0.5   # the scene covers the image
    differs = (got - ref).abs() > 1e-4 * ref.abs().clamp(min=1.0)
    assert differs.float().mean() < 1e-4, differs.float().mean()
    # a far Gaussian is not culled by a far threshold on this path (depth.py:33-41 has none)
    g2, _, _ = make_scene(64, W, H, 0, seed=5, device=DEV)
    g2.xyz[:, 2] += 1.0e4
    g2.scale[:] = 6.0
    g2.opacity[:] = 5.0
    far_ref = mirror_depth(g2, 0.5, T, cam, 0.3, 100, 3.0)
    far_got = fused.render_depth(g2, 0.5, T, cam, 0.3, 100, 3.0)
    assert (far_ref > 0).any() and torch.equal(far_got > 0, far_ref > 0)


@pytest.mark.parametrize("tag", ["deg0", "deg3_pre"])
def test_fused_matches_reference_host_fixtures(tag):
    fx = load(f"ref_host_synth_{tag}.npz")
    g, cam, T = scene_from_fixture(fx, DEV, requires_grad=True)
    img, mask, uv = fused.rasterize(g, T, cam, float(fx["near"]), float(fx["far"]), int(fx["padding"]),
                                    float(fx["mh_dist"]), True, t(fx["background"], DEV))
    uv.retain_grad()
    img.backward(t(fx["grad_image"], DEV))
    assert np.array_equal(mask.cpu().numpy(), fx["mask"])
    diff = np.abs(img.detach().cpu().numpy() - fx["image"]).max(axis=2)
    assert (diff > 1e-5).mean() < 2e-3 and diff.max() < 5e-3
    assert uv.grad is not None
    errs = {"uv": scaled_err(uv.grad, t(fx["grad_uv"]))}
    for k in PARAMS:
        if "grad_" + k in fx.files:
            errs[k] = scaled_err(getattr(g, k).grad, t(fx["grad_" + k]))
    report(f"fused_vs_reference_host_fixture[{tag}]", image_max_diff=float(diff.max()),
           pixels_over_1e5=float((diff > 1e-5).mean()), grad_scaled_err=max(errs.values()))
    assert max(errs.values()) < E2E_GRAD_TOL, errs


def test_fused_backward_parity_vs_oracle_chain():
    """dense parameter gradients of the fused backward against the oracle's per-stage backward
    kernels chained on the CPU from the same render gradients"""
    N, W, H, deg, seed = 8000, 320, 240, 3, 5
    near, far, pad, mh = 0.3, 500.0, 100, 3.0
    g, cam, T = make_scene(N, W, H, deg, seed=seed)
    exp = cpu_expected_stages(g, cam, T, near, far, pad, mh)
    gd, camd, Td = make_scene(N, W, H, deg, seed=seed, device=DEV)
    for k in PARAMS:
        getattr(gd, k).requires_grad_(True)
    bg = torch.zeros(3, device=DEV)
    image, mask, uv, aux = fused.rasterize(gd, Td, camd, near, far, pad, mh, True, bg, return_aux=True)
    for k in ("conic", "opacity", "rgb"):
        aux[k].retain_grad()
    uv.retain_grad()
    image.backward(make_grad_image(W, H, seed=3, device=DEV))
    g_uv, g_conic = uv.grad.cpu().contiguous(), aux["conic"].grad.cpu().contiguous()
    g_opa, g_rgb = aux["opacity"].grad.cpu().contiguous(), aux["rgb"].grad.cpu().contiguous()
    # oracle chain
    expect = oracle_vjp(exp, torch.cat([g_rgb, g_opa.reshape(-1, 1), g_uv, g_conic], dim=1))
    for k, e in expect.items():
        got = getattr(gd, k).grad.cpu()
        assert torch.equal(got[exp["culled"]], torch.zeros_like(got[exp["culled"]])), k
        assert scaled_err(got, e) < 2e-5, f"{k}: {scaled_err(got, e)}"


def test_fused_known_answers_and_uv_grad():
    """test/test_rasterize.py:21-54 through the fused path; uv.retain_grad() semantics"""
    g, cam, T, fx = scene6(DEV)
    for k in ("xyz", "rgb", "opacity", "scale", "quaternion"):
        getattr(g, k).requires_grad_(True)
    img, mask, uv = fused.rasterize(g, T, cam, 0.3, 100.0, 10, 3.0, True, torch.zeros(3, device=DEV))
    for ch, v in enumerate([0.47698545455932617, 0.0, 0.0]):
        assert abs(img[340, 348, ch].item() - v) < 5e-6
    for ch, v in enumerate([0.03330837935209274, 0.0, 0.267561137676239]):
        assert abs(img[200, 348, ch].item() - v) < 5e-6
    assert mask.tolist() == [True, True, True, False, False, False]
    uv.retain_grad()
    img.sum().backward()
    assert uv.grad.shape == (3, 2) and torch.isfinite(uv.grad).all() and uv.grad.abs().sum() > 0
    assert (g.xyz.grad[:3] == 0).all() and g.xyz.grad[3:].abs().sum() > 0


def test_fused_everything_culled_and_no_grad_paths():
    g, cam, T = make_scene(500, 128, 96, 0, seed=1, device=DEV)
    img, mask, uv = fused.rasterize(g, T, cam, 1000.0, 2000.0, 100, 3.0, True, torch.full((3,), 0.25, device=DEV))
    assert mask.all() and uv.shape == (0, 2)
    assert torch.allclose(img, torch.full_like(img, 0.25))
    with torch.no_grad():
        img2, _, _ = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, torch.zeros(3, device=DEV))
    assert img2.shape == (96, 128, 3)


def test_fused_tile_row_bands_tile_the_frame():
    """multi-GPU building block on one GPU: rendering the frame band by band (tile_rows) gives the
    same image bit for bit and gradients that sum to the full-frame gradients"""
    N, W, H, deg = 20000, 640, 472, 3
    bg = torch.full((3,), 0.5, device=DEV)
    gi = make_grad_image(W, H, seed=2, device=DEV)

    def run(rows):
        g, cam, T = make_scene(N, W, H, deg, seed=7, device=DEV)
        for k in PARAMS:
            getattr(g, k).requires_grad_(True)
        img, mask, uv = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg, tile_rows=rows)
        img.backward(gi)
        return img.detach(), {k: getattr(g, k).grad for k in PARAMS}

    full_img, full_g = run(None)
    nty = (H + 15) // 16
    bands = [(0, 7), (7, 19), (19, nty)]
    parts = [run(r) for r in bands]
    assert torch.equal(sum(p[0] for p in parts), full_img)
    for k in PARAMS:
        s = sum(p[1][k] for p in parts)
        assert scaled_err(s, full_g[k]) < 1e-5, k


def test_sharded_rasterizer_single_rank_rccl():
    """ShardedRasterizer over an RCCL ("nccl") process group of one rank == the plain fused path"""
    import os
    import torch.distributed as dist
    from gaussian_splatting_amd.sharded import ShardedRasterizer
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV, 0))
    try:
        bg = torch.zeros(3, device=DEV)
        gi = make_grad_image(256, 192, seed=2, device=DEV)
        outs = []
        for sharded in (False, True):
            g, cam, T = make_scene(3000, 256, 192, 3, seed=9, device=DEV)
            for k in PARAMS:
                getattr(g, k).requires_grad_(True)
            fn = ShardedRasterizer(192, 1, 0).rasterize if sharded else fused.rasterize
            img, mask, uv = fn(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg)
            img.backward(gi)
            outs.append((img.detach(), {k: getattr(g, k).grad for k in PARAMS}))
        assert torch.equal(outs[0][0], outs[1][0])
        for k in PARAMS:
            assert scaled_err(outs[1][1][k], outs[0][1][k]) < 1e-5, k
    finally:
        if created:
            dist.destroy_process_group()


def test_fused_speculative_capacity_overflow_is_repaired():
    """the emit + sort are launched with a capacity guessed from the previous frame; a too small
    guess must be detected and repaired, a too large one must not change anything"""
    bg = torch.zeros(3, device=DEV)

    def run():
        g, cam, T = make_scene(20000, 640, 480, 0, seed=3, device=DEV)
        img, _, _, aux = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg, return_aux=True)
        return img, aux["sorted_gaussians"].clone(), aux["tile_ranges"].clone()

    fused._capacity_hint.clear()
    ref = run()                                  # no hint: exact path
    assert len(fused._capacity_hint) == 1
    key = next(iter(fused._capacity_hint))
    spec = run()                                 # hint present: speculative path
    fused._capacity_hint[key] = 100              # far too small: overflow, repaired
    small = run()
    fused._capacity_hint[key] = 10 * ref[1].numel()
    large = run()
    for other in (spec, small, large):
        assert torch.equal(other[0], ref[0]) and torch.equal(other[1], ref[1]) and torch.equal(other[2], ref[2])

    # the default mode (prefix sort, render enqueued on the speculative lists before the host read):
    # a too small capacity must not be read beyond, and the frame is repeated
    def run_default():
        g, cam, T = make_scene(20000, 640, 480, 0, seed=3, device=DEV)
        g.xyz.requires_grad_(True)
        img, _, _ = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg)
        img.sum().backward()
        return img.detach(), g.xyz.grad

    for hint in (None, 100, 1500, 10 * ref[1].numel()):
        if hint is not None:
            fused._capacity_hint[key] = hint
        img, grad = run_default()
        assert torch.equal(img, ref[0]), hint
        assert torch.isfinite(grad).all()


def test_kernels_run_on_the_current_stream():
    """launches go to torch's current HIP stream, with no hidden device sync the
    caller could be relying on -- a frame issued on a side stream equals one on the default stream"""
    bg = torch.zeros(3, device=DEV)
    gi = make_grad_image(320, 240, seed=4, device=DEV)

    def run():
        g, cam, T = make_scene(8000, 320, 240, 3, seed=21, device=DEV)
        for k in PARAMS:
            getattr(g, k).requires_grad_(True)
        img, _, _ = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg)
        img.backward(gi)
        return img.detach(), g.xyz.grad

    ref_img, ref_grad = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        img, grad = run()
    side.synchronize()
    assert torch.equal(img, ref_img)
    assert scaled_err(grad, ref_grad) < 1e-5


def test_backward_hands_the_slab_through_without_a_copy(monkeypatch):
    """_Render.backward returns four views of one [V, 9] slab; _Preprocess.backward must recognise them
    (also with uv.retain_grad(), as the trainer does) and read the slab in place"""
    seen = []
    real = fused._as_slab

    def spy(g_uv, g_conic, g_opa, g_rgb, V, dev):
        out = real(g_uv, g_conic, g_opa, g_rgb, V, dev)
        seen.append(g_rgb is not None and g_rgb._base is not None and out is g_rgb._base)
        return out

    monkeypatch.setattr(fused, "_as_slab", spy)
    monkeypatch.setattr(fused, "NATIVE", False)   # the Python orchestration; the native one is checked below
    g, cam, T = make_scene(5000, 320, 240, 3, seed=5, device=DEV)
    for k in PARAMS:
        getattr(g, k).requires_grad_(True)
    img, _, uv = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, torch.zeros(3, device=DEV))
    uv.retain_grad()
    img.backward(make_grad_image(320, 240, seed=1, device=DEV))
    assert seen == [True]
    assert uv.grad is not None and uv.grad.shape == uv.shape and torch.isfinite(uv.grad).all()
    py_uv_grad = uv.grad.clone()
    # the native orchestration (csrc/frame_hip.cpp): same structure, counted by the module itself
    monkeypatch.setattr(fused, "NATIVE", True)
    nat = fused.native()
    assert nat is not None, "native frame module not built"
    nat.reset_counters()
    g, cam, T = make_scene(5000, 320, 240, 3, seed=5, device=DEV)
    for k in PARAMS:
        getattr(g, k).requires_grad_(True)
    img, _, uv = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, torch.zeros(3, device=DEV))
    uv.retain_grad()
    img.backward(make_grad_image(320, 240, seed=1, device=DEV))
    c = nat.counters()
    assert c["frames"] == 1 and c["slab_copies"] == 0
    assert uv.grad is not None and scaled_err(uv.grad, py_uv_grad) < 1e-5


def test_python_frames_release_their_memory_by_reference_count():
    """Every Python-orchestrated frame kind, with the cyclic collector off: once a frame's outputs are dropped its device
    memory is back, so torch.cuda.memory_allocated() after the third and the fourth frame are equal (frames 1 and 2
    fill the module's bounded per-shape caches: capacity hints, the pinned read ring, empties).  A frame record that
    refers to itself would keep its two arenas until the collector runs."""
    import gc
    W, H = 128, 96
    g, cam, T = make_scene(2000, W, H, 1, seed=3, device=DEV)
    leaves = [getattr(g, k).requires_grad_(True) for k in PARAMS]
    feat = torch.rand(2000, 3, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
    bg = torch.zeros(3, device=DEV)
    gi = make_grad_image(W, H, seed=1, device=DEV)
    args = (T, cam, 0.3, 500.0, 100, 3.0)

    def backward(*outputs):
        # image-like outputs [H, W, C] get gi's first C channels, maps [H, W] its first channel
        torch.autograd.backward(outputs, [gi[..., :o.shape[2]] if o.dim() == 3 else gi[..., 0] for o in outputs])

    kinds = {
        "rasterize": lambda: backward(fused.rasterize(g, *args, True, bg)[0]),
        "frame_hook": lambda: backward(fused.rasterize(g, *args, True, bg, frame_hook=lambda d: None)[0]),
        "rgbd": lambda: backward(*fused.rasterize_rgbd(g, *args, True, bg)[:3]),
        "features": lambda: backward(*fused.rasterize_features(g, feat, *args, True, bg)[:3]),
        "per_pixel_sh": lambda: backward(fused.rasterize(g, *args, False, bg)[0]),
        "contributions": lambda: fused.rasterize_contributions(g, *args, True, bg),
    }
    prev = fused.NATIVE
    fused.NATIVE = False
    gc.collect()
    gc.disable()
    try:
        for name, frame in kinds.items():
            seen = []
            for _ in range(4):
                frame()
                for x in leaves + [feat]:
                    x.grad = None
                fused.reset_counters()
                fused.last_flags(clear=True)
                torch.cuda.synchronize()
                seen.append(torch.cuda.memory_allocated())
            print(f"[python frame memory] {name}: {seen}")
            assert seen[2] == seen[3], (name, seen)
    finally:
        gc.enable()
        fused.NATIVE = prev


@pytest.mark.parametrize("deg,bgval", [(0, 0.0), (3, 0.5)])
def test_native_orchestration_equals_python_orchestration(deg, bgval):
    """csrc/frame_hip.cpp against fused.py's own stages: same kernels in the same order -> image and
    culling mask bit-identical, gradients equal up to the atomics' order; also on a tile-row band"""
    N, W, H = 20000, 640, 472
    bg = torch.full((3,), bgval, device=DEV)
    gi = make_grad_image(W, H, seed=4, device=DEV)
    for rows in (None, (5, 19)):
        outs = []
        for native in (False, True):
            fused.NATIVE = native
            try:
                g, cam, T = make_scene(N, W, H, deg, seed=2, device=DEV)
                for k in PARAMS:
                    if getattr(g, k) is not None:
                        getattr(g, k).requires_grad_(True)
                img, mask, uv = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg, tile_rows=rows)
                uv.retain_grad()
                img.backward(gi)
            finally:
                fused.NATIVE = True
            outs.append((img.detach(), mask, uv.detach(), uv.grad, {k: getattr(g, k).grad for k in PARAMS
                                                                      if getattr(g, k) is not None}))
        (i0, m0, u0, gu0, p0), (i1, m1, u1, gu1, p1) = outs
        assert torch.equal(i0, i1) and torch.equal(m0, m1) and torch.equal(u0, u1)
        assert scaled_err(gu1, gu0) < 1e-5
        for k in p0:
            assert scaled_err(p1[k], p0[k]) < 1e-5, k


@pytest.mark.parametrize("case,N", [("short", 20_000), ("medium", 90_000), ("long", 400_000)])
def test_native_frame_guesses_the_longest_list(case, N):
    """Complete-list frames of the native orchestration guess the frame's LONGEST tile list from the shape's last
    frame: "none beyond the prefix" leaves the render's repair phase out, "none beyond 4096" the sort's walk-grid
    kernel (workload B otherwise pays for three launches that find nothing to do).  The count pass reports the true
    value with the frame's counts; every wrong guess must be made good -- the repair enqueued late, or the frame's
    emit + sort + render repeated -- and the results stay those of the Python orchestration, which guesses nothing."""
    nat = fused.native()
    if nat is None:
        pytest.skip("native frame module not built")
    W, H = 256, 192
    g, cam, T = make_scene(N, W, H, 0, seed=9, device=DEV)
    if case != "short":
        g.opacity.fill_(-5.0)   # faint: pixels composite thousands of entries, prefix-sorted tiles ARE flagged
    bg = torch.full((3,), 0.25, device=DEV)
    gi = make_grad_image(W, H, seed=3, device=DEV)
    for k in PARAMS:
        if getattr(g, k) is not None:
            getattr(g, k).requires_grad_(True)

    def frame(native):
        prev = fused.NATIVE, fused.DEPTH_CUT
        fused.NATIVE, fused.DEPTH_CUT = native, False
        try:
            for k in PARAMS:
                if getattr(g, k) is not None:
                    getattr(g, k).grad = None
            img, mask, uv = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg)
            img.backward(gi)
            return img.detach().clone(), {k: getattr(g, k).grad.clone() for k in PARAMS if getattr(g, k) is not None}
        finally:
            fused.NATIVE, fused.DEPTH_CUT = prev

    def same(a, b):
        assert torch.equal(a[0], b[0])
        for k in b[1]:
            assert scaled_err(a[1][k], b[1][k]) < 1e-5, k

    # the longest list of this scene, from the Python stages
    f = fused.preprocess_forward(g.xyz.detach(), g.quaternion.detach(), g.scale.detach(), g.opacity.detach(), g.rgb.detach(),
                                 None, T, cam.K, W, H, 0.3, 500.0, 100, 3.0, None, 0)
    longest = int((f.ranges[1:] - f.ranges[:-1]).max())
    lo, hi = {"short": (1, 1024), "medium": (1025, 4096), "long": (4097, 10 ** 9)}[case]
    assert lo <= longest <= hi, (case, longest)
    ref = frame(False)
    fused.reset_counters()
    same(frame(True), ref)                 # first frame of the shape: nothing guessed
    same(frame(True), ref)                 # guess = the truth
    c0 = fused.counters()
    for hint in (100, 2000, 10 ** 6, 100):
        nat.debug_set_longest_list_hints(hint)
        same(frame(True), ref)
    c = fused.counters()
    report(f"longest_list_guess[{case}]", longest=longest,
           **{k: c.get(k, -1) for k in ("prefix_frames_without_repair_launches", "prefix_late_repairs", "long_list_misses",
                                        "capacity_misses", "speculative_frames")})
    if case == "short":
        assert c0["prefix_frames_without_repair_launches"] >= 1 and c["prefix_late_repairs"] == 0 and c["long_list_misses"] == 0, c
    elif case == "medium":
        assert c0["prefix_frames_without_repair_launches"] == 0, c0
        assert c["prefix_late_repairs"] >= 2 and c["long_list_misses"] == 0, c   # the two frames that guessed 100
    else:
        assert c["long_list_misses"] >= 3, c   # guesses 100, 2000, 100 of a frame with a list beyond 4096


def test_native_frame_kinds_share_one_record_per_shape():
    """The native orchestration keeps ONE record of guesses per frame shape (csrc/frame_policy.h: ShapeState): row-
    restricted frames, whole complete-list frames and whole depth-cut frames of a scene in alternation.  The second
    frame of every (shape, mode) must run on guessed capacities and none may miss -- a cut frame's capacity is its KEPT
    count, far below the complete count the uncut frame of the same shape needs, so the two must not overwrite each
    other -- and every result stays that of the Python orchestration, which guesses nothing."""
    nat = fused.native()
    if nat is None:
        pytest.skip("native frame module not built")
    N, W, H = 90_000, 256, 192   # the "medium" scene of test_native_frame_guesses_the_longest_list
    g, cam, T = make_scene(N, W, H, 0, seed=9, device=DEV)
    g.opacity.fill_(-5.0)
    bg = torch.full((3,), 0.25, device=DEV)
    gi = make_grad_image(W, H, seed=3, device=DEV)
    for k in PARAMS:
        if getattr(g, k) is not None:
            getattr(g, k).requires_grad_(True)

    def frame(native, cut, rows):
        prev = fused.NATIVE, fused.DEPTH_CUT
        fused.NATIVE, fused.DEPTH_CUT = native, cut
        try:
            for k in PARAMS:
                if getattr(g, k) is not None:
                    getattr(g, k).grad = None
            img, mask, uv = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg, tile_rows=rows)
            img.backward(gi)
            return img.detach().clone(), {k: getattr(g, k).grad.clone() for k in PARAMS if getattr(g, k) is not None}
        finally:
            fused.NATIVE, fused.DEPTH_CUT = prev

    refs = {rows: frame(False, False, rows) for rows in ((3, 9), None)}
    fused.reset_counters()
    seen, log = set(), []
    for cut, rows in ((False, (3, 9)), (False, (3, 9)), (True, None), (False, None), (True, None), (False, None)):
        before = fused.counters()
        img, grads = frame(True, cut, rows)
        c = fused.counters()
        d = {k: c[k] - before[k] for k in ("frames", "speculative_frames", "capacity_misses", "depth_cut_frames")}
        log.append(d)
        assert d["frames"] == 1 and d["depth_cut_frames"] == int(cut), (cut, rows, d)
        if (cut, rows) in seen:
            assert d["speculative_frames"] == 1, (cut, rows, d)
        seen.add((cut, rows))
        assert torch.equal(img, refs[rows][0]), (cut, rows)
        for k in grads:
            assert scaled_err(grads[k], refs[rows][1][k]) < 1e-5, (cut, rows, k)
    c = fused.counters()
    report("native_frame_shared_records", S_min=c["S_min"], S_max=c["S_max"],
           speculative=[d["speculative_frames"] for d in log], misses=[d["capacity_misses"] for d in log])
    assert c["frames"] == 6 and c["capacity_misses"] == 0 and c["depth_cut_frames"] == 2, c


def test_fused_rasterize_rejects_bad_inputs():
    """the fused path hands raw pointers to the C ABI: wrong dtype / device / shape must raise like the
    reference's TORCH_CHECKs (src/checks.cuh:5-14) instead of reading garbage"""
    N, W, H = 500, 128, 96
    bg = torch.zeros(3, device=DEV)

    def scene():
        return make_scene(N, W, H, 3, seed=1, device=DEV)

    g, cam, T = scene()
    fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg)   # the good case
    def set_attr(obj, name, value):
        setattr(obj, name, value)   # (the Gaussians constructor asserts shapes itself: break the tensor afterwards)
        return obj

    for breakage, match in (
            (lambda g, cam, T: (g, cam, T.double()), "camera_T_world is not a float tensor"),
            (lambda g, cam, T: (g, type(cam)(cam.width, cam.height, cam.K.double()), T), "K is not a float tensor"),
            (lambda g, cam, T: (g, cam, T.cpu()), "camera_T_world is not a CUDA tensor"),
            (lambda g, cam, T: (set_attr(g, "quaternion", g.quaternion[:, :3].contiguous()), cam, T),
             "quaternion must have shape"),
            (lambda g, cam, T: (set_attr(g, "opacity", g.opacity.view(-1)), cam, T), "opacity must have shape"),
            (lambda g, cam, T: (set_attr(g, "scale", g.scale.double()), cam, T), "scale is not a float tensor"),
            (lambda g, cam, T: (set_attr(g, "sh", g.sh[:, :, :7].contiguous()), cam, T), "sh must have shape")):
        g, cam, T = scene()
        g2, cam2, T2 = breakage(g, cam, T)
        with pytest.raises(RuntimeError, match=match):
            fused.rasterize(g2, T2, cam2, 0.3, 500.0, 100, 3.0, True, bg)
    with pytest.raises(RuntimeError, match="background_rgb is not a CUDA tensor"):
        g, cam, T = scene()
        fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg.cpu())


@pytest.mark.parametrize("N,W,H,deg,seed,tilt", [(20000, 640, 472, 3, 1, False), (20000, 640, 472, 3, 1, True),
                                                 (60000, 640, 472, 0, 2, True), (30000, 1280, 720, 1, 3, True)])
def test_end_to_end_difference_is_flipped_threshold_decisions(N, W, H, deg, seed, tilt):
    """What the 5e-3 end-to-end bound above is made of.  The fused path and the reference's host pipeline
    compute the per-splat render inputs with ulp-level differences (explicit fp32 world->camera
    expression vs a BLAS matmul, torch.sigmoid vs the kernel's, torch.inverse vs an fp64 inverse).  An
    ulp in a splat's alpha flips the `alpha >= 1/255` test (or the saturation test) at a few pixels, each
    flip worth up to 1/255 of a colour.  Fingerprint every pixel's decisions -- splats visited before
    saturation, splats that passed the alpha test -- with the oracle on both sets of inputs: away from
    the pixels whose fingerprint differs, image and gradients agree to 1e-5, not 5e-3."""
    from gaussian_splatting_amd import backend, splat_cuda
    from gaussian_splatting_amd.splat_py.utils import transform_points_torch

    orc = oracle()
    near, far, pad, mh = 0.3, 500.0, 100, 3.0
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    gi = make_grad_image(W, H, seed=seed + 9)
    pose = torch.eye(4)
    if tilt:    # a general rotation: the world->camera products are no longer exact in either pipeline
        pose[:3, :3] = torch.tensor([[0.9999, 0.0089, 0.0073], [-0.0106, 0.9568, 0.2905], [-0.0044, -0.2906, 0.9568]])
        pose[:3, 3] = torch.tensor([0.05, -0.1, 0.3])
    c = lambda x: x.detach().cpu().contiguous()

    def fingerprint(uv, opacity, rgb, conic, ranges, sorted_g):
        img, nsp, fw = torch.zeros(H, W, 3), torch.zeros(H, W, dtype=torch.int32), torch.zeros(H, W)
        cnt = orc.render_tiles_with_contrib_count(uv, opacity, rgb, conic, torch.zeros(1, 1, 1), ranges, sorted_g,
                                                  torch.full((3,), 0.5), nsp, fw, img)
        return img, nsp, cnt

    # the reference's host pipeline on the CPU (mirror + oracle kernels); its render inputs are captured
    cap = {}

    def capture(rgb, opacity, uv, conic):
        cap.update(rgb=c(rgb), opacity=c(opacity), uv=c(uv), conic=c(conic))
        return rgb, opacity, uv, conic

    backend.use(orc)
    try:
        g, cam, T = make_scene(N, W, H, deg, seed=seed)
        T = (pose @ T).contiguous()
        params = [k for k in PARAMS if getattr(g, k) is not None]
        for k in params:
            getattr(g, k).requires_grad_(True)
        img_ref, mask_ref, _ = rasterize_mirror(g, T, cam, near, far, pad, mh, True, torch.full((3,), 0.5),
                                                grad_sync=capture)
        xyz_c = transform_points_torch(g.xyz.detach(), T)[~mask_ref].contiguous()
        sorted_ref, ranges_ref = orc.get_sorted_gaussian_list(1024, cap["uv"], xyz_c, cap["conic"], ntx, nty, mh)
        fp_ref = fingerprint(cap["uv"], cap["opacity"], cap["rgb"], cap["conic"], ranges_ref, sorted_ref)
        assert torch.equal(fp_ref[0], img_ref.detach())

        # the fused path on the GPU; its render inputs are read back
        gd, camd, _ = make_scene(N, W, H, deg, seed=seed, device=DEV)
        Td = T.to(DEV)
        for k in params:
            getattr(gd, k).requires_grad_(True)
        img_gpu, mask_gpu, uv_gpu, aux = fused.rasterize(gd, Td, camd, near, far, pad, mh, True,
                                                         torch.full((3,), 0.5, device=DEV), return_aux=True)
        assert torch.equal(mask_gpu.cpu(), mask_ref)
        fp_gpu = fingerprint(c(uv_gpu), c(aux["opacity"]), c(aux["rgb"]), c(aux["conic"]), c(aux["tile_ranges"]),
                             c(aux["sorted_gaussians"]))
        assert (fp_gpu[0] - c(img_gpu)).abs().max() < 1e-5       # the HIP render of those inputs == the oracle's

        ulp = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
        input_diff = {k: ulp(x, cap[k]) for k, x in (("uv", c(uv_gpu)), ("opacity", c(aux["opacity"])),
                                                     ("rgb", c(aux["rgb"])), ("conic", c(aux["conic"])))}
        assert max(input_diff.values()) < 1e-3, input_diff

        flipped = (fp_ref[1] != fp_gpu[1]) | (fp_ref[2] != fp_gpu[2])
        same = ~flipped
        diff = (c(img_gpu) - img_ref.detach()).abs().amax(dim=2)
        frac = flipped.float().mean().item()
        assert frac < 5e-3, frac
        assert diff.max() < 5e-3                                   # the bound of the tests above, all pixels
        assert diff[same].max() < 1e-5, diff[same].max()           # ... and where no decision flipped

        # gradients with the flipped pixels taken out of the loss: the same 20k-Gaussian frame agrees to 1e-5
        gi_masked = gi * same.unsqueeze(2)
        img_ref.backward(gi_masked)
        img_gpu.backward(gi_masked.to(DEV))
        errs = {k: scaled_err(getattr(gd, k).grad, getattr(g, k).grad) for k in params}
        assert max(errs.values()) < 2e-5, errs
        report(f"end_to_end_flipped_decisions[{N}-{W}x{H}-deg{deg}-tilt{int(tilt)}]", flipped_pixel_fraction=frac, flipped_pixels=int(flipped.sum()),
               image_max_diff_all=diff.max().item(), image_max_diff_unflipped=diff[same].max().item(),
               max_scaled_input_diff=max(input_diff.values()), grad_scaled_err_unflipped=max(errs.values()))
    finally:
        backend.use(splat_cuda)


@pytest.mark.parametrize("W,H", [(1024, 592), (1040, 592)])   # 2368 tiles (a multiple of 8) and 2405 (not)
def test_backward_longest_first_tile_order(W, H, monkeypatch):
    """gs_render_tiles_backward_slab with the forward's tile costs: the launch order is a permutation of the
    tiles, by non-increasing cost class within each XCD's eighth of the frame, and the gradients are those of
    the natural order (the atomics' summation order is the only difference)"""
    import ctypes

    from gaussian_splatting_amd import _hip
    N = 60000                                        # >= 2048 tiles: the order is used
    monkeypatch.setattr(fused, "LPT_MIN_MEAN_LIST", 0)   # ... whatever the mean list length
    g, cam, T = make_scene(N, W, H, 0, seed=5, device=DEV)
    bg = torch.zeros(3, device=DEV)
    gi = make_grad_image(W, H, seed=6, device=DEV)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, 0.3, 500.0, 100,
                                 3.0, None, _hip.GS_SORT_PREFIX)
    V = f.V
    rgb_v = f.rgb_render[:V]
    image, nsp, fw, cost, _ = fused.render_forward(f.packed, rgb_v, f.ranges, f.sorted_g, f.keys, bg, H, W, None,
                                                   _hip.GS_SORT_PREFIX, segments=False)
    nt = ((W + 15) // 16) * ((H + 15) // 16)
    assert cost.shape == (nt,) and int(cost.min()) > 0
    natural = fused.render_backward(f.packed, rgb_v, f.ranges, f.sorted_g, bg, nsp, fw, gi, H, W, None, V)
    ordered = fused.render_backward(f.packed, rgb_v, f.ranges, f.sorted_g, bg, nsp, fw, gi, H, W, None, V, cost)
    for j in range(9):
        assert scaled_err(ordered[:, j], natural[:, j]) < 2e-6, j
    # the order itself
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    order = torch.full((nt + 8,), -7, dtype=torch.int32, device=DEV)
    # zero_slab_rows = V: the call clears the slab itself (in the launch that makes the order) -- rows beyond stay
    big = torch.full((V + 3, 9), 7.0, device=DEV)
    slab = big[:V]
    _hip.call("gs_render_tiles_backward_slab", p(f.packed), p(rgb_v), p(f.ranges), p(f.sorted_g), p(bg), p(nsp), p(fw),
              p(gi), W, H, 0, (H + 15) // 16, p(slab), ctypes.c_int64(V), p(cost), p(order), None, None, None, None,
              _hip.GS_BACKWARD_DEFAULT, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (big[V:] == 7.0).all()
    # ... also without an order (fill-only prologue), and zero_slab_rows = 0 accumulates onto what is there
    again = torch.full((V, 9), 3.0, device=DEV)
    _hip.call("gs_render_tiles_backward_slab", p(f.packed), p(rgb_v), p(f.ranges), p(f.sorted_g), p(bg), p(nsp), p(fw),
              p(gi), W, H, 0, (H + 15) // 16, p(again), ctypes.c_int64(V), None, None, None, None, None, None,
              _hip.GS_BACKWARD_DEFAULT, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert scaled_err(again, natural) < 2e-6
    _hip.call("gs_render_tiles_backward_slab", p(f.packed), p(rgb_v), p(f.ranges), p(f.sorted_g), p(bg), p(nsp), p(fw),
              p(gi), W, H, 0, (H + 15) // 16, p(again), ctypes.c_int64(0), None, None, None, None, None, None,
              _hip.GS_BACKWARD_DEFAULT, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert scaled_err(again, 2 * natural) < 4e-6
    n_grid = (nt + 7) // 8 * 8                       # the launch grid; block 8 j + x is the j-th tile of XCD x
    per = n_grid // 8

    def check_order(order_t):
        o = order_t.cpu()
        assert sorted(t for t in o[:n_grid].tolist() if t >= 0) == list(range(nt)) and (o[n_grid:] == -7).all()
        for x in range(8):
            mine = o[x:n_grid:8]
            tiles = mine[mine >= 0]
            assert (mine[len(tiles):] == -1).all()                      # idle blocks come last
            assert ((tiles // per) == x).all()                          # the XCD keeps its contiguous eighth
            c = cost.cpu()[tiles.long()].float()
            cls = (c * (127.0 / float(cost.max()))).int()               # the kernel's cost classes
            assert (cls[1:] <= cls[:-1]).all()

    check_order(order)
    assert scaled_err(slab, natural) < 2e-6
    # the prologue as its own call (what the fused frames do): the same order, the slab cleared; the backward then
    # takes the order as given
    order2 = torch.full((nt + 8,), -7, dtype=torch.int32, device=DEV)
    slab2 = torch.full((V, 9), 5.0, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _hip.call("gs_render_backward_prologue", p(slab2), ctypes.c_int64(V), p(cost), p(order2), W, H, 0, (H + 15) // 16, stream)
    check_order(order2)   # (tiles of one cost class come in the order the LDS atomics hand out: not repeatable)
    assert not slab2.any()
    _hip.call("gs_render_tiles_backward_slab", p(f.packed), p(rgb_v), p(f.ranges), p(f.sorted_g), p(bg), p(nsp), p(fw),
              p(gi), W, H, 0, (H + 15) // 16, p(slab2), ctypes.c_int64(0), None, p(order2), None, None, None, None,
              _hip.GS_BACKWARD_DEFAULT, stream)
    assert scaled_err(slab2, natural) < 2e-6
    # a row range below 2048 tiles: the prologue spells out the natural order (block 8 j + x = j-th tile of eighth x)
    rows = 8
    nt_b = rows * ((W + 15) // 16)
    ng_b = (nt_b + 7) // 8 * 8
    order3 = torch.full((nt + 8,), -7, dtype=torch.int32, device=DEV)
    _hip.call("gs_render_backward_prologue", None, ctypes.c_int64(0), p(cost), p(order3), W, H, 2, 2 + rows, stream)
    o3 = order3.cpu()
    per_b = ng_b // 8
    want = torch.tensor([(b % 8) * per_b + b // 8 for b in range(ng_b)], dtype=torch.int32)
    assert torch.equal(o3[:ng_b], torch.where(want < nt_b, want, torch.full_like(want, -1))) and (o3[ng_b:] == -7).all()
    # cost without order is refused
    with pytest.raises(RuntimeError, match="go together"):
        _hip.call("gs_render_tiles_backward_slab", p(f.packed), p(rgb_v), p(f.ranges), p(f.sorted_g), p(bg), p(nsp),
                  p(fw), p(gi), W, H, 0, (H + 15) // 16, p(slab), ctypes.c_int64(0), p(cost), None, None, None, None, None,
                  _hip.GS_BACKWARD_DEFAULT,
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    # the gradient mode is an argument of the call (ABI 5): anything but DEFAULT / COMPAT / EXACT is refused
    with pytest.raises(RuntimeError, match="backward mode"):
        _hip.call("gs_render_tiles_backward_slab", p(f.packed), p(rgb_v), p(f.ranges), p(f.sorted_g), p(bg), p(nsp),
                  p(fw), p(gi), W, H, 0, (H + 15) // 16, p(slab), ctypes.c_int64(0), None, None, None, None, None, None, 7,
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_second_backward_over_a_retained_graph():
    """every backward pass accumulates into a fresh zeroed slab: a second pass over a retained graph doubles the
    parameter gradients, it does not add onto the first pass's slab.  (Zero-filling the slab on a side stream
    during the forward, so that the backward need not, was tried: the frame got 3-5 % SLOWER at B, C and D.)"""
    N, W, H = 20000, 320, 240
    bg = torch.zeros(3, device=DEV)
    gi = make_grad_image(W, H, seed=3, device=DEV)
    g, cam, T = make_scene(N, W, H, 1, seed=4, device=DEV)
    for k in PARAMS:
        getattr(g, k).requires_grad_(True)
    img, _, _ = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg)
    img.backward(gi, retain_graph=True)
    once = {k: getattr(g, k).grad.clone() for k in PARAMS}
    img.backward(gi)
    for k in PARAMS:
        assert scaled_err(getattr(g, k).grad, 2 * once[k]) < 2e-6, k


@pytest.mark.parametrize("deg", [0, 1])
def test_packed_render_entry_points_equal_the_reference_signature_ones(deg):
    """gs_render_tiles_packed / gs_render_tiles_backward_packed (records of gs_pack_splats) against
    gs_render_tiles / gs_render_tiles_backward (the reference's argument lists, record formed while staging):
    the same kernels on the same record values -- images bit-equal, gradients equal up to the atomics' order"""
    import ctypes

    from gaussian_splatting_amd import _hip, splat_cuda
    N, W, H = 8000, 200, 152
    g, cam, T = make_scene(N, W, H, deg, seed=11, device=DEV)
    bg = torch.full((3,), 0.25, device=DEV)
    gi = make_grad_image(W, H, seed=12, device=DEV)
    img0, mask, uv, aux = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, bg, return_aux=True)
    uv, opa, rgb, conic = uv.detach().contiguous(), aux["opacity"].contiguous(), aux["rgb"].contiguous(), aux["conic"].contiguous()
    ranges, sorted_g = aux["tile_ranges"], aux["sorted_gaussians"]
    V = uv.shape[0]
    rays = torch.zeros(1, 1, 1, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = _hip.current_stream()
    nty = (H + 15) // 16

    def outputs():
        return (torch.zeros(H, W, dtype=torch.int32, device=DEV), torch.zeros(H, W, device=DEV), torch.zeros(H, W, 3, device=DEV))

    def grads():
        return [torch.zeros_like(x) for x in (rgb, opa, uv, conic)]

    nsp_a, fw_a, img_a = outputs()
    splat_cuda.render_tiles_cuda(uv, opa, rgb, conic, rays, ranges, sorted_g, bg, nsp_a, fw_a, img_a)
    ga = grads()
    splat_cuda.render_tiles_backward_cuda(uv, opa, rgb, conic, rays, ranges, sorted_g, bg, nsp_a, fw_a, gi, *ga)

    packed = torch.empty(V, 12, device=DEV)
    _hip.call("gs_pack_splats", p(uv), p(opa), p(conic), p(rgb), V, p(packed), _hip.GS_F32, stream)
    nsp_b, fw_b, img_b = outputs()
    _hip.call("gs_render_tiles_packed", p(packed), p(rgb), p(rays), p(ranges), p(sorted_g), p(bg), W, H, 1, 0, nty,
              p(nsp_b), p(fw_b), p(img_b), _hip.GS_F32, None, stream)
    gb = grads()
    _hip.call("gs_render_tiles_backward_packed", p(packed), p(rgb), p(rays), p(ranges), p(sorted_g), p(bg), p(nsp_b),
              p(fw_b), p(gi), W, H, 1, 0, nty, p(gb[0]), p(gb[1]), p(gb[2]), p(gb[3]), _hip.GS_F32,
              _hip.GS_BACKWARD_COMPAT, stream)
    assert torch.equal(img_a, img_b) and torch.equal(nsp_a, nsp_b) and torch.equal(fw_a, fw_b)
    assert torch.equal(img_a, img0.detach())
    for a, b in zip(ga, gb):
        assert scaled_err(b, a) < 2e-6


@pytest.mark.parametrize("dtype,n_sh", [(torch.float32, 16), (torch.float64, 1), (torch.float64, 16)])
def test_general_forward_staging_forms_and_bands(dtype, n_sh):
    """k_render_fwd_general (every forward but fp32 with one coefficient) rendered three ways: gs_render_tiles on the
    separate arrays (record formed while staging), gs_render_tiles_packed on records of gs_pack_splats, and the latter
    in two calls over the tile rows [0, 1) and [1, nty) into one set of buffers.  The same kernel on the same record
    values, no atomics: num_splats, final weight and image bit-equal.  faint_300: one tile, 300 faint splats that no
    pixel saturates on (the CPU oracle walks all 300 at every pixel) -- 5 chunks of 64 with a partial last one at 16
    coefficients, 256 + 44 in fp64 with one.  partial_48x40: 3 x 3 tiles, partial right and bottom tiles, empty tiles
    and single-entry ones."""
    import ctypes

    from gaussian_splatting_amd import _hip

    from . import render_ref64 as R
    gs_dtype = _hip.GS_F32 if dtype == torch.float32 else _hip.GS_F64
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    stream = _hip.current_stream()
    for name in ("faint_300", "partial_48x40"):
        sc = R.render_scenes()[name]
        W, H, V, nty = sc.W, sc.H, sc.V, (sc.H + 15) // 16
        rays = (sc.rays if n_sh > 1 else torch.zeros(1, 1, 1)).to(dtype)
        uv, opa, coeff, conic, bg = (x.to(dtype).contiguous() for x in (sc.uv, sc.opacity, R.scene_coeff(sc, n_sh),
                                                                        sc.conic, sc.bg))
        if name == "faint_300":
            nsp, fw, img = torch.zeros(H, W, dtype=torch.int32), torch.zeros(H, W, dtype=dtype), torch.zeros(H, W, 3, dtype=dtype)
            oracle().render_tiles_cuda(uv, opa, coeff, conic, rays, sc.ranges, sc.sorted_g, bg, nsp, fw, img)
            assert (nsp == 300).all()   # the last, partial chunk is reached by every pixel
        uv, opa, coeff, conic, bg, rays, ranges, sorted_g = (x.to(DEV) for x in (uv, opa, coeff, conic, bg, rays, sc.ranges,
                                                                                 sc.sorted_g))

        def outputs():
            return (torch.zeros(H, W, dtype=torch.int32, device=DEV), torch.zeros(H, W, dtype=dtype, device=DEV),
                    torch.zeros(H, W, 3, dtype=dtype, device=DEV))

        nsp_a, fw_a, img_a = outputs()
        _hip.call("gs_render_tiles", p(uv), p(opa), p(coeff), p(conic), p(rays), p(ranges), p(sorted_g), p(bg), p(nsp_a),
                  p(fw_a), p(img_a), W, H, n_sh, 0, nty, gs_dtype, stream)
        packed = torch.empty(V, 12, dtype=dtype, device=DEV)
        _hip.call("gs_pack_splats", p(uv), p(opa), p(conic), p(coeff if n_sh == 1 else None), V, p(packed), gs_dtype, stream)
        nsp_b, fw_b, img_b = outputs()
        _hip.call("gs_render_tiles_packed", p(packed), p(coeff), p(rays), p(ranges), p(sorted_g), p(bg), W, H, n_sh, 0, nty,
                  p(nsp_b), p(fw_b), p(img_b), gs_dtype, None, stream)
        nsp_c, fw_c, img_c = outputs()
        for row0, row1 in ((0, 1), (1, nty)):
            _hip.call("gs_render_tiles_packed", p(packed), p(coeff), p(rays), p(ranges), p(sorted_g), p(bg), W, H, n_sh, row0,
                      row1, p(nsp_c), p(fw_c), p(img_c), gs_dtype, None, stream)
        assert int(nsp_a.max()) > 0 and bool(img_a.any())
        for got in ((nsp_b, fw_b, img_b), (nsp_c, fw_c, img_c)):
            assert torch.equal(nsp_a, got[0]) and torch.equal(fw_a, got[1]) and torch.equal(img_a, got[2]), name


@pytest.mark.parametrize("mode", ["compat", "exact"])
@pytest.mark.parametrize("n_sh", [4, 16])
def test_per_pixel_sh_backward_staging_forms_and_bands(n_sh, mode):
    """k_render_bwd_sh (fp32 with per-pixel SH) run three ways after one gs_render_tiles forward, each into freshly
    zeroed gradient arrays: gs_render_tiles_backward on the separate arrays (record formed while staging),
    gs_render_tiles_backward_packed on records of gs_pack_splats, and the latter in two calls over the tile rows [0, 1)
    and [1, nty) into one set of arrays.  The same kernel on the same record values under another order of atomics:
    the four gradients within scaled_err < 2e-6 of the first form (the bound of
    test_packed_render_entry_points_equal_the_reference_signature_ones), rows of Gaussians that are in no list exactly
    zero, every gradient tensor with a non-zero entry.  faint_300: one tile, 300 faint splats every pixel walks to the
    end -- five 64-entry chunks with a partial last one, batches of 16 that close in mid-chunk.  partial_48x40: 3 x 3
    tiles, partial right and bottom tiles, empty tiles and single-entry lists.  The first form is the yardstick of the
    other two; of its own values this test checks only the non-zero entry and the zero rows, and their correctness
    rests on tests/test_gpu_render_ref64.py (the first form against the fp64 reference on these scenes)."""
    import ctypes

    from gaussian_splatting_amd import _hip

    from . import render_ref64 as R
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    stream = _hip.current_stream()
    gs_mode = _hip.GS_BACKWARD_EXACT if mode == "exact" else _hip.GS_BACKWARD_COMPAT
    for name in ("faint_300", "partial_48x40"):
        sc = R.render_scenes()[name]
        W, H, V, nty = sc.W, sc.H, sc.V, (sc.H + 15) // 16
        uv, opa, coeff, conic, bg, rays, gi, ranges, sorted_g = (
            x.contiguous().to(DEV) for x in (sc.uv, sc.opacity, R.scene_coeff(sc, n_sh), sc.conic, sc.bg, sc.rays,
                                             sc.grad_image, sc.ranges, sc.sorted_g))
        nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
        fw, img = torch.zeros(H, W, device=DEV), torch.zeros(H, W, 3, device=DEV)
        _hip.call("gs_render_tiles", p(uv), p(opa), p(coeff), p(conic), p(rays), p(ranges), p(sorted_g), p(bg), p(nsp),
                  p(fw), p(img), W, H, n_sh, 0, nty, _hip.GS_F32, stream)
        if name == "faint_300":
            assert bool((nsp == 300).all())   # the last, partial chunk is reached by every pixel
        packed = torch.empty(V, 12, device=DEV)
        _hip.call("gs_pack_splats", p(uv), p(opa), p(conic), None, V, p(packed), _hip.GS_F32, stream)

        def grads():
            return [torch.zeros_like(x) for x in (coeff, opa, uv, conic)]

        def backward_packed(g, row0, row1):
            _hip.call("gs_render_tiles_backward_packed", p(packed), p(coeff), p(rays), p(ranges), p(sorted_g), p(bg),
                      p(nsp), p(fw), p(gi), W, H, n_sh, row0, row1, p(g[0]), p(g[1]), p(g[2]), p(g[3]), _hip.GS_F32,
                      gs_mode, stream)

        ga, gb, gc = grads(), grads(), grads()
        _hip.call("gs_render_tiles_backward", p(uv), p(opa), p(coeff), p(conic), p(rays), p(ranges), p(sorted_g), p(bg),
                  p(nsp), p(fw), p(gi), p(ga[0]), p(ga[1]), p(ga[2]), p(ga[3]), W, H, n_sh, 0, nty, _hip.GS_F32, gs_mode,
                  stream)
        backward_packed(gb, 0, nty)
        backward_packed(gc, 0, 1)
        backward_packed(gc, 1, nty)

        listed = torch.zeros(V, dtype=torch.bool, device=DEV)
        listed[sorted_g[:int(ranges[-1])].long()] = True
        for form, got in (("separate", ga), ("packed", gb), ("packed_bands", gc)):
            for key, a, b in zip(R.GRAD_KEYS, ga, got):
                assert bool(b.any()), (name, form, key)
                assert not bool(b[~listed].any()), (name, form, key)
                if got is not ga:
                    err = scaled_err(b, a)
                    report("per_pixel_sh_backward_forms", scene=name, n_sh=n_sh, mode=mode, form=form, grad=key,
                           scaled_err=err)
                    assert err < 2e-6, (name, form, key, err)
