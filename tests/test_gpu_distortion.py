"""The depth-distortion map: gs_render_distortion / gs_render_distortion_backward and fused.rasterize_distortion against
the float64 reference of tests/distortion_ref.py (held to what this file needs by tests/test_distortion_ref.py on the
CPU).  The scenes keep their seeded, unsorted z: the kernels are held to the LIST-ORDER definition.

Rules (the measures and bounds of tests/test_gpu_render_ref64.py, unchanged: R_MAX = 8, NOISE_MARGIN = 2e-5):
  forward    on the non-fragile pixels |got - ref| / (|fp32 restatement - ref| + 2^-24 abs_p + 2^-22 |ref|) <= R_MAX;
             depth, alpha and transmittance torch.equal to gs_render_zalpha's
  gradients  noise_measure(kernel) <= noise_measure(fp32 restatement) + NOISE_MARGIN per tensor (g_z, g_opacity, g_uv,
             g_conic) against the true derivative; rows no pixel uses exactly zero; slab columns 0..2 as they were
  NULL       a NULL gradient is a gradient of zeros: one tile, the same bits; several tiles, the sums of a row arrive in
             another order, within (tiles - 1) x 2^-24 of the terms' magnitudes
  no g_dist  one tile: slab and grad_z torch.equal to gs_render_zalpha_backward's
  a slab that also holds the colour backward's gradient: per element |got - ref| <= B_c abs_c + B_d abs_d, the colour
             rule's bound (oracle's walk measure + 2e-5) on the colour part's magnitudes plus this file's on the maps'

Measured on an MI355X (every case leaves its figures in the parity report):
  kernels, eight scenes   r_distortion 0.44 (opaque_stack) to 1.98 (long_1100); fragile 0 %
             gradients    kernel 3.9e-6 at most (long_1100, g_z; restatement 1.4e-6), 8.2e-7 at most on the slab's columns
                          (long_1100, g_conic; restatement 2.2e-7), 5.1e-7 at most on the other scenes
             NULL         several tiles: 1.4e-9 at most (strip_70x13, g_uv) against 2.4e-7; one tile: the same bits, and
                          without g_dist the bits of gs_render_zalpha_backward
  frame (shift -5.5)      r_distortion 1.73, 0.03 % of the pixels fragile; distortion == pairwise form within the reference
             loss on distortion   error / bound 0.16 at most (g_z), 0.024 on the slab's columns
             loss on all four     error / bound 0.16 (g_z), 0.041 at most on the slab's columns (colour bounds 3.3e-5 to 3.6e-5)
  image-only loss         parameter gradients within 1.7e-6 (rel_err) of fused.rasterize's
  pose, distortion loss   r 0.023"""
import functools

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS

from . import depth_alpha_ref as D
from . import distortion_ref as X
from . import render_ref64 as R
from .helpers import rel_err, report
from .pose_terms import pose_r, pose_reference
from .test_gpu_depth_alpha import calls_of, fp32_fma_close, frame_case, frame_inputs, param_grads, slab_fields
from .test_gpu_render_ref64 import FRAME, NOISE_MARGIN, R_MAX, frame_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCENES = list(R.render_scenes())
SHIFT = FRAME["shift"]


# ---- 1. the kernels against the reference -----------------------------------------------------------------------------
def kernel_run(sc, grads, pattern=None, zalpha=False):
    """the depth scene through gs_pack_splats, gs_render_tiles_packed (for num_splats_per_pixel), gs_render_zalpha,
    gs_render_distortion and gs_render_distortion_backward -> dict of CPU tensors; grads: (g_dist, g_depth, g_alpha),
    each [H, W] or None (NULL); pattern [V, 3]: what the slab's columns 0..2 hold before the call; zalpha: the backward
    is gs_render_zalpha_backward with (g_depth, g_alpha) instead"""
    c = lambda x: x.to(DEV).float().contiguous() if x.is_floating_point() else x.to(DEV).contiguous()
    V, W, H = sc.V, sc.W, sc.H
    nty = (H + 15) // 16
    s = _hip.current_stream()
    p = _hip.ptr
    uv, opacity, conic, rgb = c(sc.uv), c(sc.opacity), c(sc.conic), c(sc.coeff16[:, :, 0])
    ranges, sorted_g, bg = c(sc.ranges), c(sc.sorted_g), c(sc.bg)
    packed = torch.empty(V, 12, device=DEV)
    _hip.call("gs_pack_splats", p(uv), p(opacity), p(conic), p(rgb), V, p(packed), _hip.GS_F32, s)
    image = torch.zeros(H, W, 3, device=DEV)
    fw = torch.zeros(H, W, device=DEV)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    _hip.call("gs_render_tiles_packed", p(packed), p(rgb), None, p(ranges), p(sorted_g), p(bg), W, H, 1, 0, nty, p(nsp),
              p(fw), p(image), _hip.GS_F32, None, s)
    xyz_cam = torch.zeros(V, 3, device=DEV)
    xyz_cam[:, 2] = sc.z.to(DEV)
    nan = lambda: torch.full((H, W), float("nan"), device=DEV)
    zd, za, zt = nan(), nan(), nan()
    _hip.call("gs_render_zalpha", p(packed), p(xyz_cam), p(ranges), p(sorted_g), p(nsp), W, H, 0, nty, p(zd), p(za), p(zt), s)
    dist, depth, alpha, t_end = nan(), nan(), nan(), nan()
    _hip.call("gs_render_distortion", p(packed), p(xyz_cam), p(ranges), p(sorted_g), p(nsp), W, H, 0, nty, p(dist),
              p(depth), p(alpha), p(t_end), s)
    slab = torch.zeros(V, 9, device=DEV)
    if pattern is not None:
        slab[:, :3] = pattern.to(DEV)
    g_z = torch.zeros(V, device=DEV)
    gx, gd, ga = (None if g is None else c(g) for g in grads)
    if zalpha:
        _hip.call("gs_render_zalpha_backward", p(packed), p(xyz_cam), p(ranges), p(sorted_g), p(nsp), p(zt), p(gd), p(ga),
                  W, H, 0, nty, p(slab), p(g_z), s)
    else:
        _hip.call("gs_render_distortion_backward", p(packed), p(xyz_cam), p(ranges), p(sorted_g), p(nsp), p(t_end),
                  p(depth), p(alpha), p(gx), p(gd), p(ga), W, H, 0, nty, p(slab), p(g_z), s)
    slab = slab.cpu()
    return dict(nsp=nsp.cpu(), distortion=dist.cpu(), depth=depth.cpu(), alpha=alpha.cpu(), t_end=t_end.cpu(),
                zalpha=(zd.cpu(), za.cpu(), zt.cpu()), colour=slab[:, :3], g_z=g_z.cpu(),
                g_opacity=slab[:, fused.SLAB_OPACITY], g_uv=slab[:, fused.SLAB_UV], g_conic=slab[:, fused.SLAB_CONIC])


def gradient_measures(vals, got, ref):
    """-> the rule's right-hand side per tensor; the measures of the kernel and of the restatement go into vals"""
    bounds = {}
    for k in X.KEYS:
        vals[f"restatement_{k}"] = X.noise_measure(ref.rest[k], ref.grad[k], ref.abs[k])
        vals[f"kernel_{k}"] = X.noise_measure(got[k], ref.grad[k], ref.abs[k])
        bounds[k] = vals[f"restatement_{k}"] + NOISE_MARGIN
    return bounds


def gradient_verdict(vals, got, ref, bounds):
    for k in X.KEYS:
        assert vals[f"kernel_{k}"] <= bounds[k], (k, vals)
        assert not got[k][~ref.used].any(), k                 # rows no pixel uses: exactly zero
        assert got[k][ref.used].abs().max() > 0, k


@pytest.mark.parametrize("name", SCENES)
def test_kernels_against_the_reference(name):
    sc, ref = D.depth_scene(name), X.reference(name)
    ok = ~ref.fragile
    gi = ref.grad_image.float()
    grads = (gi[..., 0], gi[..., 1], gi[..., 2])
    pattern = torch.randn(sc.V, 3, generator=torch.Generator().manual_seed(3))
    got = kernel_run(sc, grads, pattern)
    assert torch.equal(got["colour"], pattern)                    # the slab's columns 0..2 as they were
    assert torch.equal(got["nsp"][ok], ref.nsp[ok])
    for k, z in zip(("depth", "alpha", "t_end"), got["zalpha"]):
        assert bool(torch.isfinite(got[k]).all()), k              # every pixel of the frame is written
        assert torch.equal(got[k], z), k                          # the depth kernel's bits
    assert bool(torch.isfinite(got["distortion"]).all())
    vals = {"fragile": float(ref.fragile.float().mean()), "r_distortion": X.forward_ratio(got["distortion"], ref, ok)}
    bounds = gradient_measures(vals, got, ref)
    # NULL = zeros, for each of the three gradients
    zero = torch.zeros(sc.H, sc.W)
    tiles = sc.ranges.numel() - 1
    for i, which in enumerate(("distortion", "depth", "alpha")):
        a = kernel_run(sc, tuple(None if j == i else g for j, g in enumerate(grads)))
        b = kernel_run(sc, tuple(zero if j == i else g for j, g in enumerate(grads)))
        for k in X.KEYS:
            if tiles == 1:
                assert torch.equal(a[k], b[k]), (which, k)
            else:
                m = X.noise_measure(a[k], b[k], ref.abs[k])
                vals[f"null_{which}_{k}"] = m
                assert m <= (tiles - 1) * 2.0 ** -24, (which, k, m)
        assert a["g_opacity"].abs().max() > 0
        if which == "distortion" and tiles == 1:
            # without g_dist the kernel is the depth backward: the fma forms make g_dist = 0 exact
            zb = kernel_run(sc, grads, zalpha=True)
            for k in X.KEYS:
                assert torch.equal(a[k], zb[k]), ("no g_dist", k)
    report(f"distortion_kernels[{name}]", **vals)
    print(f"distortion_kernels[{name}]: {vals}")
    assert vals["r_distortion"] <= R_MAX, vals
    gradient_verdict(vals, got, ref, bounds)


def test_kernel_entry_points_validate():
    """bad arguments are GS_EINVAL with a message; all gradients NULL and empty lists launch nothing harmful"""
    z = torch.zeros(4, device=DEV)
    lib, s = _hip.lib(), _hip.current_stream()
    p = _hip.ptr
    assert lib.gs_render_distortion(None, None, None, None, None, 0, 16, 0, 1, p(z), p(z), p(z), p(z), s) == _hip.GS_EINVAL
    assert b"non-empty" in lib.gs_last_error()
    assert lib.gs_render_distortion(None, None, p(z), None, p(z), 16, 16, 0, 2, p(z), p(z), p(z), p(z), s) == _hip.GS_EINVAL
    assert b"tile row" in lib.gs_last_error()
    assert lib.gs_render_distortion(None, None, p(z), None, p(z), 16, 16, 0, 1, None, p(z), p(z), p(z), s) == _hip.GS_EINVAL
    assert b"render_distortion: an output is NULL" in lib.gs_last_error()
    assert lib.gs_render_distortion_backward(None, None, p(z), None, p(z), None, p(z), p(z), None, None, None, 16, 16, 0,
                                             1, None, None, s) == _hip.GS_EINVAL
    assert lib.gs_render_distortion_backward(None, None, p(z), None, p(z), p(z), None, p(z), None, None, None, 16, 16, 0,
                                             1, None, None, s) == _hip.GS_EINVAL
    assert b"depth or alpha is NULL" in lib.gs_last_error()
    # empty lists, V == 0: zeros and a transmittance of one; the backward adds nothing
    W, H = 33, 17
    ranges = torch.zeros(3 * 2 + 1, dtype=torch.int32, device=DEV)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    x, d, a, t = (torch.full((H, W), 7.0, device=DEV) for _ in range(4))
    e = torch.empty(0, device=DEV)
    _hip.call("gs_render_distortion", p(e), p(e), p(ranges), p(e), p(nsp), W, H, 0, 2, p(x), p(d), p(a), p(t), s)
    assert not x.any() and not d.any() and not a.any() and bool((t == 1).all())
    slab, gz = torch.ones(1, 9, device=DEV), torch.ones(1, device=DEV)
    one = torch.ones(H, W, device=DEV)
    _hip.call("gs_render_distortion_backward", p(e), p(e), p(ranges), p(e), p(nsp), p(t), p(d), p(a), p(one), p(one),
              p(one), W, H, 0, 2, p(slab), p(gz), s)
    _hip.call("gs_render_distortion_backward", p(e), p(e), p(ranges), p(e), p(nsp), p(t), p(d), p(a), None, None, None,
              W, H, 0, 2, None, None, s)
    assert bool((slab == 1).all()) and bool((gz == 1).all())


# ---- 2. the frame -----------------------------------------------------------------------------------------------------
def distortion_frame(g, T, cam, bg, **kw):
    return fused.rasterize_distortion(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS, **kw)


@functools.lru_cache(maxsize=None)
def frame_reference_distortion():
    """the distortion reference on the frame's own complete lists (tests/test_gpu_depth_alpha.py's frame_case: a
    return_aux frame of fused.rasterize) for a seeded (g_dist, g_depth, g_alpha); once"""
    case = frame_case(SHIFT)
    gen = torch.Generator().manual_seed(FRAME["seed"] + 3)
    gi = torch.randn(FRAME["H"], FRAME["W"], 3, generator=gen)
    return X.reference_of(case.sc, gi, case.ref.fragile, case.ref.nsp)


frame_cache = {}


def test_frame_outputs():
    """image / culling_mask / uv bit-equal to fused.rasterize's, depth / alpha to rasterize_rgbd's (antialiased off and
    on), distortion against the reference on the frame's own lists, which within the reference is the pairwise form"""
    case, ref = frame_case(SHIFT), frame_reference_distortion()
    ok = ~ref.fragile
    pair = X.pairwise(case.sc, ref.decisions)
    assert float((ref.distortion - pair).abs().max()) <= 1e-12 * float(pair.max())
    for aa in (False, True):
        g, cam, T, bg = frame_inputs(SHIFT, grads=False)
        image, depth, alpha, dist, mask, uv = distortion_frame(g, T, cam, bg, antialiased=aa)
        want = fused.rasterize_rgbd(g, T, cam, use_sh_precompute=True, background_rgb=bg, antialiased=aa, **DEFAULTS)
        plain = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, antialiased=aa, **DEFAULTS)
        assert torch.equal(image, plain[0]) and torch.equal(mask, plain[1]) and torch.equal(uv, plain[2]), aa
        assert torch.equal(depth, want[1]) and torch.equal(alpha, want[2]), aa
        assert tuple(dist.shape) == (FRAME["H"], FRAME["W"]) and bool(torch.isfinite(dist).all())
        if not aa:
            assert torch.equal(image.cpu(), case.image) and torch.equal(uv.cpu(), case.uv)
            r = X.forward_ratio(dist.cpu(), ref, ok)
            report("distortion_frame[forward]", r_distortion=r, fragile=float(ref.fragile.float().mean()))
            print(f"distortion_frame: r_distortion = {r:.3g}")
            assert r <= R_MAX, r
        else:
            assert not torch.equal(dist.cpu(), frame_cache["plain"])   # the antialiased opacity reaches the weights
        frame_cache["plain" if not aa else "aa"] = dist.cpu()


@pytest.mark.parametrize("loss", ["distortion", "all"])
def test_frame_slab_and_parameter_gradients(loss):
    """a loss on distortion alone / on all four outputs: the kept slab and last_grad_z() against the reference by the
    combined-slab rule, then the parameter gradients against fused.preprocess_backward on the kept slab plus the z term"""
    case, ref = frame_case(SHIFT), frame_reference_distortion()
    sc = case.sc
    W, H = sc.W, sc.H
    gi = ref.grad_image.float()
    if loss == "distortion":
        zero = torch.zeros(H, W, 3)
        zero[..., 0] = gi[..., 0]
        want = X.reference_of(sc, zero, ref.fragile, ref.nsp)
        cref = None
    else:
        want = ref
        csc, cref, corc = frame_reference()
        assert torch.equal(csc.uv, sc.uv) and torch.equal(csc.sorted_g, sc.sorted_g)
    g, cam, T, bg = frame_inputs(SHIFT)
    fused.keep_last_slab(True)
    try:
        _hip.set_backward_mode("exact")
        outs = {}

        def run():
            image, depth, alpha, dist, mask, uv = distortion_frame(g, T, cam, bg)
            outs.update(image=image, dist=dist)
            gx, gd, ga = (want.grad_image[..., i].float().to(DEV) for i in range(3))
            if loss == "distortion":
                torch.autograd.backward([dist], [gx])
            else:
                torch.autograd.backward([dist, depth, alpha, image], [gx, gd, ga, cref.grad_image.float().to(DEV)])

        calls = calls_of(run)
        slab, g_z = fused.last_slab(), fused.last_grad_z()
    finally:
        _hip.set_backward_mode("compat")
        fused.keep_last_slab(False)
    # one map forward and one map backward, never the depth kernels beside them
    assert "gs_render_zalpha" not in calls and "gs_render_zalpha_backward" not in calls
    assert len(calls["gs_render_distortion"]) == 1 and len(calls["gs_render_distortion_backward"]) == 1
    assert len(calls.get("gs_render_tiles_backward_slab", [])) == (0 if loss == "distortion" else 1)
    assert len(calls["gs_z_backward"]) == 1
    assert torch.equal(outs["image"].detach().cpu(), case.image)
    assert slab is not None and g_z is not None and tuple(slab.shape) == (sc.V, 9) and tuple(g_z.shape) == (sc.V,)
    got = slab_fields(slab.cpu(), g_z.cpu())
    vals = {}
    used = want.used.clone()
    for k in X.KEYS:
        b_d = X.noise_measure(want.rest[k], want.grad[k], want.abs[k]) + NOISE_MARGIN
        target, bound = want.grad[k], b_d * want.abs[k]
        vals[f"restatement_{k}"] = b_d - NOISE_MARGIN
        if cref is not None and k != "g_z":
            b_c = D.noise_measure(corc[k], cref.grad_walk[k], cref.abs_walk[k]) + NOISE_MARGIN
            target = target + cref.grad_walk[k]
            bound = bound + b_c * cref.abs_walk[k]
            vals[f"colour_bound_{k}"] = b_c
        err = (got[k].double().reshape(target.shape) - target).abs()
        live = bound > 0
        vals[f"kernel_over_bound_{k}"] = float((err[live] / bound[live]).max())
    if cref is not None:
        used |= cref.used
    report(f"distortion_frame[loss {loss}]", **vals)
    print(f"distortion_frame[loss {loss}]: {vals}")
    for k in X.KEYS:
        assert vals[f"kernel_over_bound_{k}"] <= 1.0, (k, vals)
        assert not got[k][~used].any(), k
        assert got[k][used].abs().max() > 0, k
    if loss == "distortion":
        assert not slab[:, :3].any()
    # the per-Gaussian node: the kept slab through fused.preprocess_backward on a fresh record, plus the z term
    g2, cam2, T2, _ = frame_inputs(SHIFT, grads=False)
    f = fused.preprocess_forward(g2.xyz, g2.quaternion, g2.scale, g2.opacity, g2.rgb, g2.sh, T2, cam2.K, W, H,
                                 DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"],
                                 DEFAULTS["mh_dist"], None, 0)
    assert f.V == sc.V
    gx_, gq, gs, go, gc, gsh = fused.preprocess_backward(g2.xyz, g2.quaternion, g2.scale, T2, cam2.K, f, slab.contiguous())
    for k, w in (("quaternion", gq), ("scale", gs), ("opacity", go), ("rgb", gc), ("sh", gsh)):
        if getattr(g, k) is not None:
            assert torch.equal(getattr(g, k).grad, w), k
    rank = f.rank.cpu().long()
    z_term = torch.zeros(FRAME["N"], 3, dtype=torch.float64)
    vis = rank >= 0
    z_term[vis] = g_z.double().cpu()[rank[vis]][:, None] * T2.double().cpu()[2, :3][None, :]
    assert fp32_fma_close(g.xyz.grad, gx_, z_term)
    assert bool((g.xyz.grad.cpu()[vis] != gx_.cpu()[vis]).any())


def test_frame_image_only_loss_costs_no_map_backward():
    """a loss on the image alone: the parameter gradients of fused.rasterize (another order of the atomics, nothing
    else) and no map backward launch; a loss on alpha alone: the map backward, no colour backward, no z backward"""
    w = torch.randn(FRAME["H"], FRAME["W"], 3, generator=torch.Generator().manual_seed(12)).to(DEV)
    g, cam, T, bg = frame_inputs(SHIFT)
    image, mask, uv = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
    (image * w).sum().backward()
    want = param_grads(g)
    g, cam, T, bg = frame_inputs(SHIFT)
    out = {}
    calls = calls_of(lambda: out.update(image=distortion_frame(g, T, cam, bg)[0]) or (out["image"] * w).sum().backward())
    assert torch.equal(out["image"].detach(), image.detach())
    assert "gs_render_distortion_backward" not in calls and "gs_z_backward" not in calls
    assert "gs_render_zalpha" not in calls and "gs_render_zalpha_backward" not in calls
    assert len(calls["gs_render_distortion"]) == 1 and len(calls["gs_render_tiles_backward_slab"]) == 1
    vals = {}
    for k, a in param_grads(g).items():
        vals[k] = rel_err(a, want[k])
        assert vals[k] < 1e-4, (k, vals[k])
    report("distortion_frame_image_only", **vals)
    g, cam, T, bg = frame_inputs(SHIFT)
    calls = calls_of(lambda: distortion_frame(g, T, cam, bg)[2].sum().backward())
    assert "gs_render_tiles_backward_slab" not in calls and "gs_z_backward" not in calls
    assert len(calls["gs_render_backward_prologue"]) == 1 and len(calls["gs_render_distortion_backward"]) == 1
    for k, a in param_grads(g).items():
        assert bool(torch.isfinite(a).all()), k
        assert (k == "rgb") != bool(a.any()), k     # the colour has no part in alpha


def test_frame_with_nothing_visible():
    g, cam, T, bg = frame_inputs(0.0)
    image, depth, alpha, dist, mask, uv = fused.rasterize_distortion(g, T, cam, 0.1, 0.2, 100, 3.0, True, bg)
    assert uv.shape[0] == 0 and bool(mask.all())
    assert tuple(dist.shape) == (FRAME["H"], FRAME["W"]) and not dist.any() and not depth.any() and not alpha.any()
    (dist.sum() + depth.sum() + alpha.sum() + image.sum()).backward()
    for k, a in param_grads(g).items():
        assert not a.any(), k


# ---- 3. the pose ------------------------------------------------------------------------------------------------------
def test_pose_gradient_of_a_distortion_loss():
    """the frame with camera_T_world requiring a gradient, loss on distortion alone: T.grad against the closed form of
    tests/pose_terms.py on the kept slab plus the float64 sum of the direct term of z = T[2, 0:3] . xyz + T[2, 3] on
    the kept g_z; pose_r with the z term's |t64| and |t32 - t64| added to B and E, as the depth-loss pose case"""
    g, cam, T, bg = frame_inputs(SHIFT)
    T.requires_grad_(True)
    w = torch.randn(FRAME["H"], FRAME["W"], generator=torch.Generator().manual_seed(4)).to(DEV)
    fused.keep_last_slab(True)
    try:
        image, depth, alpha, dist, mask, uv = distortion_frame(g, T, cam, bg)
        (dist * w).sum().backward()
        slab, g_z = fused.last_slab(), fused.last_grad_z()
    finally:
        fused.keep_last_slab(False)
    assert slab is not None and g_z is not None and not slab[:, :3].any()
    vis = torch.nonzero(~mask.cpu()).flatten()
    c = lambda x: x.detach().cpu()
    xyz_v = c(g.xyz)[vis]
    ref, B, E = pose_reference(xyz_v, c(g.quaternion)[vis], c(g.scale)[vis], c(T), c(cam.K), c(slab))
    gz = c(g_z)
    t64 = torch.zeros(vis.numel(), 3, 4, dtype=torch.float64)
    t64[:, 2, :3] = gz.double()[:, None] * xyz_v.double()
    t64[:, 2, 3] = gz.double()
    t32 = torch.zeros(vis.numel(), 3, 4)
    t32[:, 2, :3] = gz[:, None] * xyz_v
    t32[:, 2, 3] = gz
    ref, B, E = ref + t64.sum(0), B + t64.abs().sum(0), E + (t32.double() - t64).abs().sum(0)
    assert T.grad is not None and tuple(T.grad.shape) == (4, 4) and bool(torch.isfinite(T.grad).all())
    assert not T.grad[3].any()
    r = pose_r(T.grad, ref, B, E)
    report("distortion_pose[distortion loss]", r=r)
    print(f"distortion_pose: r = {r:.3g}")
    assert r <= R_MAX, r
    assert bool(t64.sum(0)[2].abs().max() > 0)


# ---- 4. the guards ----------------------------------------------------------------------------------------------------
def test_guards_raise_before_anything_is_enqueued():
    g, cam, T, bg = frame_inputs(0.0, grads=False)
    args = (g, T, cam, DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"], DEFAULTS["mh_dist"])
    sh = torch.zeros(FRAME["N"], 3, 3, device=DEV)
    g_sh = type(g)(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, sh)
    g_f64 = type(g)(g.xyz.double(), g.rgb.double(), g.opacity.double(), g.scale.double(), g.quaternion.double(), None)
    bad = [
        ("tile_rows", lambda: fused.rasterize_distortion(*args, True, bg, tile_rows=(0, 2))),
        ("return_aux", lambda: fused.rasterize_distortion(*args, True, bg, return_aux=True)),
        ("slab_sync", lambda: fused.rasterize_distortion(*args, True, bg, slab_sync=lambda flat: None)),
        ("frame_hook", lambda: fused.rasterize_distortion(*args, True, bg, frame_hook=lambda d: None)),
        ("adam_plan", lambda: fused.rasterize_distortion(*args, True, bg, adam_plan=object())),
        ("per-pixel SH", lambda: fused.rasterize_distortion(g_sh, *args[1:], False, bg)),
        ("float", lambda: fused.rasterize_distortion(g_f64, T.double(), type(cam)(cam.width, cam.height, cam.K.double()),
                                                     *args[3:], True, bg.double())),
    ]
    for words, call in bad:
        _hip.enable_timing(True)
        try:
            with pytest.raises(RuntimeError, match=words):
                call()
            assert not _hip.collect_timing(), words   # no entry point was called
        finally:
            _hip.enable_timing(False)
    # SH with the precompute mode is supported
    image, depth, alpha, dist, mask, uv = fused.rasterize_distortion(g_sh, *args[1:], True, bg)
    assert bool(torch.isfinite(image).all()) and bool(torch.isfinite(dist).all())
