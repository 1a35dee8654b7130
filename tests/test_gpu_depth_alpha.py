"""Differentiable depth and alpha maps: gs_render_zalpha / gs_render_zalpha_backward / gs_z_backward and
fused.rasterize_rgbd against tests/render_ref64.py fed z as a colour (tests/depth_alpha_ref.py; the inputs are held to
what this file needs by tests/test_depth_alpha_ref.py on the CPU).

Rules (the measures and bounds of tests/test_gpu_render_ref64.py, unchanged):
  forward    on the non-fragile pixels, ref64.r_measure of depth and of alpha with env = |fp32 oracle - reference| <= 8
  (a)        grad_depth / grad_alpha only on the pixels whose reference walk is not scaled (scale == 1), where the fp32
             oracle's gradient is the true derivative: noise_measure of the kernel per tensor <= the oracle's + 2e-5
  (b)        all non-fragile pixels against the TRUE derivative `grad`: the same number as (a)'s bound for that scene
             and tensor (the same arithmetic on more pixels; the oracle has no baseline there, it returns the walk
             gradient, which tests/test_depth_alpha_ref.py shows to be 2.7e-3 or more away)
  a slab that also holds the colour backward's gradient (the frame test, loss on all three outputs): per element
             |got - ref| <= |colour part's error| + |depth part's error| <= B_c abs_c + B_d abs_d with B_c the colour
             rule's bound (oracle's walk measure + 2e-5, tests/test_gpu_render_ref64.py) and B_d rule (b)'s, so the
             measure against ref = grad_walk(colour) + grad(depth), abs = abs_c + abs_d is held to max(B_c, B_d)
  gs_z_backward and the z term of xyz.grad: one fp32 rounding of the fused multiply-add, |got - exact| <= 2^-24 |exact|

Measured on an MI355X (every case leaves its figures in the parity report):
  kernels, eight scenes   r_depth 0.38 to 1.85, r_alpha 0.37 to 2.11 (both long_1100); fragile 0 %, scaled pixels 0 to 57 %
             rule (a)     kernel 6.2e-6 at most (long_1100, g_z; oracle 6.4e-6), 4.5e-7 at most on the other scenes;
                          opaque_stack: kernel 1.2e-7 where the oracle, which starts from 1 - A, has 3.3e-4
             rule (b)     kernel 3.2e-6 at most (long_1100, g_z)
             T_end        within 1.4e-6 (relative) of the float64 product in opaque_stack, 1.2e-6 elsewhere
  frame, shift -5.5       r_depth 2.0, r_alpha 2.1; combined slab 4.4e-6 (g_opacity) against bounds of 3.3e-5 to 3.6e-5,
                          g_z 2.0e-6 against 3.2e-5; 96 % of the pixels scaled
  frame, shift 0          r_depth 1.5, r_alpha 1.7; slab and g_z 1.4e-6 at most (oracle on its unscaled pixels: 8.3e-4)
  image-only loss         parameter gradients within 2.5e-6 (rel_err) of fused.rasterize's
  pose, depth loss        r 4.5 (the direct z term is 99 % of row 2)"""
import functools
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

from . import depth_alpha_ref as D
from . import render_ref64 as R
from .helpers import rel_err, report
from .pose_terms import pose_r, pose_reference
from .ref64 import general_camera_scene, r_measure, to_device
from .test_gpu_render_ref64 import FRAME, NOISE_MARGIN, R_MAX, frame_reference
from .test_render_ref64 import oracle_run

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCENES = list(R.render_scenes())
PARAMS = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")


# ---- 1. the kernels against the reference -----------------------------------------------------------------------------
def kernel_run(sc, grad_depth, grad_alpha, pattern=None):
    """the depth scene through gs_pack_splats, gs_render_tiles_packed (for num_splats_per_pixel), gs_render_zalpha and
    gs_render_zalpha_backward -> dict of CPU tensors; grad_depth / grad_alpha: [H, W] or None (NULL);
    pattern [V, 3]: what the slab's columns 0..2 hold before the call"""
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
    depth, alpha, t_end = (torch.full((H, W), float("nan"), device=DEV) for _ in range(3))
    _hip.call("gs_render_zalpha", p(packed), p(xyz_cam), p(ranges), p(sorted_g), p(nsp), W, H, 0, nty, p(depth), p(alpha),
              p(t_end), s)
    slab = torch.zeros(V, 9, device=DEV)
    if pattern is not None:
        slab[:, :3] = pattern.to(DEV)
    g_z = torch.zeros(V, device=DEV)
    gd = None if grad_depth is None else c(grad_depth)
    ga = None if grad_alpha is None else c(grad_alpha)
    _hip.call("gs_render_zalpha_backward", p(packed), p(xyz_cam), p(ranges), p(sorted_g), p(nsp), p(t_end), p(gd), p(ga),
              W, H, 0, nty, p(slab), p(g_z), s)
    slab = slab.cpu()
    return dict(nsp=nsp.cpu(), depth=depth.cpu(), alpha=alpha.cpu(), t_end=t_end.cpu(), colour=slab[:, :3],
                image=image.cpu(), g_z=g_z.cpu(), g_opacity=slab[:, fused.SLAB_OPACITY], g_uv=slab[:, fused.SLAB_UV],
                g_conic=slab[:, fused.SLAB_CONIC])


def forward_measures(got, orc, ref, ok):
    n = int(ok.sum())
    pick = lambda x: x.double()[ok].reshape(n, 1)
    return {f"r_{k}": r_measure(pick(got[k]), pick(getattr(ref, k)), pick(orc[k]) - pick(getattr(ref, k)))
            for k in ("depth", "alpha")}


def oracle_bounds(vals, sc, true):
    """rule (a)'s right-hand side per tensor: the fp32 oracle's measure on the unscaled pixels + NOISE_MARGIN"""
    orc = D.fields(oracle_run(sc, 1, torch.float32, true.grad_image, exact=True))
    for k in D.KEYS:
        vals[f"a_oracle_{k}"] = D.noise_measure(orc[k], true.grad[k], true.abs[k])
    return orc, {k: vals[f"a_oracle_{k}"] + NOISE_MARGIN for k in D.KEYS}


def check_rule(vals, tag, got, want, bounds):
    for k in D.KEYS:
        vals[f"{tag}_kernel_{k}"] = D.noise_measure(got[k], want.grad[k], want.abs[k])

    def verdict():
        for k in D.KEYS:
            assert vals[f"{tag}_kernel_{k}"] <= bounds[k], (tag, k, vals)
            assert not got[k][~want.used].any(), (tag, k)         # rows no pixel uses: exactly zero
            assert got[k][want.used].abs().max() > 0, (tag, k)
    return verdict


@pytest.mark.parametrize("name", SCENES)
def test_kernels_against_the_reference(name):
    sc = D.depth_scene(name)
    ref, true = D.reference(name), D.reference(name, True)
    ok = ~ref.fragile
    vals = {"scaled_pixels": float((ref.scale != 1).float().mean()), "fragile": float(ref.fragile.float().mean())}
    orc, bounds = oracle_bounds(vals, sc, true)
    gen = torch.Generator().manual_seed(3)
    pattern = torch.randn(sc.V, 3, generator=gen)
    runs = {}
    for tag, r in (("a", true), ("b", ref)):
        gi = r.grad_image.float()
        runs[tag] = kernel_run(sc, gi[..., 0], gi[..., 1], pattern)
        assert torch.equal(runs[tag]["colour"], pattern), tag         # the slab's columns 0..2 as they were
    got = runs["b"]
    assert torch.equal(got["nsp"][ok], ref.nsp[ok])
    for k in ("depth", "alpha", "t_end"):
        assert bool(torch.isfinite(got[k]).all()), k                  # every pixel of the frame is written
    vals.update(forward_measures(got, orc, ref, ok))
    verdicts = [check_rule(vals, "a", runs["a"], true, bounds), check_rule(vals, "b", runs["b"], ref, bounds)]
    # T_end is stored itself: 1 - alpha formed in fp32 at T ~ 1e-5 would be off by 6e-8 / 1e-5 = 6e-3, while a product
    # of <= 12 factors (1 - alpha), each carrying alpha's few ulp magnified by alpha / (1 - alpha) <= 50, stays within
    # 12 x 50 x 2^-22 = 1.4e-4 of the exact one
    t_ref = (1 - ref.alpha)[ok]
    vals["t_end_rel"] = float(((got["t_end"].double()[ok] - t_ref).abs() / t_ref).max())
    # NULL = zeros, for either gradient (one tile: one atomic per row, the same bits; several tiles: the sums of a row
    # arrive in another order, (tiles - 1) x 2^-24 of the terms' magnitudes, 9 tiles at most here)
    gi = ref.grad_image.float()
    zero = torch.zeros(sc.H, sc.W)
    one_tile = sc.ranges.numel() == 2
    for which, null, zeros in (("depth", (None, gi[..., 1]), (zero, gi[..., 1])), ("alpha", (gi[..., 0], None), (gi[..., 0], zero))):
        a, b = kernel_run(sc, *null), kernel_run(sc, *zeros)
        for k in D.KEYS:
            if one_tile:
                assert torch.equal(a[k], b[k]), (which, k)
            else:
                assert D.noise_measure(a[k], b[k], ref.abs[k]) <= 1e-6, (which, k)
        assert (which == "alpha" or not a["g_z"].any()) and a["g_opacity"].abs().max() > 0
    report(f"depth_alpha_kernels[{name}]", **vals)
    assert vals["r_depth"] <= R_MAX and vals["r_alpha"] <= R_MAX, vals
    if name == "opaque_stack":
        assert vals["t_end_rel"] <= 1e-3, vals
    for v in verdicts:
        v()


def test_kernel_entry_points_validate():
    """bad arguments are GS_EINVAL with a message; both gradients NULL, zero tile rows and empty lists launch nothing
    harmful"""
    sc = D.depth_scene("partial_33x17")
    z = torch.zeros(4, device=DEV)
    lib, s = _hip.lib(), _hip.current_stream()
    p = _hip.ptr
    assert lib.gs_render_zalpha(None, None, None, None, None, 0, 16, 0, 1, p(z), p(z), p(z), s) == _hip.GS_EINVAL
    assert b"non-empty" in lib.gs_last_error()
    assert lib.gs_render_zalpha(None, None, p(z), None, p(z), 16, 16, 0, 2, p(z), p(z), p(z), s) == _hip.GS_EINVAL
    assert b"tile row" in lib.gs_last_error()
    assert lib.gs_render_zalpha_backward(None, None, p(z), None, p(z), None, None, None, 16, 16, 0, 1, None, None,
                                         s) == _hip.GS_EINVAL
    # empty lists, V == 0: zeros and a transmittance of one; the backward adds nothing
    W, H = 33, 17
    ranges = torch.zeros(3 * 2 + 1, dtype=torch.int32, device=DEV)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    d, a, t = (torch.full((H, W), 7.0, device=DEV) for _ in range(3))
    e = torch.empty(0, device=DEV)
    _hip.call("gs_render_zalpha", p(e), p(e), p(ranges), p(e), p(nsp), W, H, 0, 2, p(d), p(a), p(t), s)
    assert not d.any() and not a.any() and bool((t == 1).all())
    slab, gz = torch.ones(1, 9, device=DEV), torch.ones(1, device=DEV)
    _hip.call("gs_render_zalpha_backward", p(e), p(e), p(ranges), p(e), p(nsp), p(t), p(d), p(a), W, H, 0, 2, p(slab),
              p(gz), s)
    _hip.call("gs_render_zalpha_backward", p(e), p(e), p(ranges), p(e), p(nsp), p(t), None, None, W, H, 0, 2, None, None, s)
    assert bool((slab == 1).all()) and bool((gz == 1).all())
    # tile rows: only the rows asked for are written
    got = kernel_run(sc, None, torch.ones(sc.H, sc.W))
    c = lambda x: x.to(DEV).contiguous()
    packed = torch.empty(sc.V, 12, device=DEV)
    uv, opacity, conic = c(sc.uv), c(sc.opacity), c(sc.conic)   # (held: a temporary's block is reused by the next one)
    ranges, sorted_g, nsp = c(sc.ranges), c(sc.sorted_g), c(got["nsp"])
    _hip.call("gs_pack_splats", p(uv), p(opacity), p(conic), None, sc.V, p(packed), _hip.GS_F32, s)
    xyz_cam = torch.zeros(sc.V, 3, device=DEV)
    xyz_cam[:, 2] = sc.z.to(DEV)
    d, a, t = (torch.full((sc.H, sc.W), 7.0, device=DEV) for _ in range(3))
    _hip.call("gs_render_zalpha", p(packed), p(xyz_cam), p(ranges), p(sorted_g), p(nsp), sc.W, sc.H, 1, 2, p(d), p(a),
              p(t), s)
    assert bool((d[:16] == 7).all()) and torch.equal(d[16:].cpu(), got["depth"][16:])
    assert torch.equal(a[16:].cpu(), got["alpha"][16:])


# ---- 2. gs_z_backward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 200, 70_000])
def test_z_backward(N):
    gen = torch.Generator().manual_seed(40 + N % 7)
    v_base = 13
    culled = torch.rand(N, generator=gen) < 0.3
    V = int((~culled).sum())
    rank = torch.full((N,), -1, dtype=torch.int32)
    rank[~culled] = v_base + torch.randperm(V, generator=gen).int()
    g_z = torch.randn(V, generator=gen) * 10.0 ** (-4 * torch.rand(V, generator=gen))
    T = torch.randn(4, 4, generator=gen)          # no orthonormality assumed
    before = torch.randn(N, 3, generator=gen)
    grad_xyz, d_rank, d_gz, d_T = before.to(DEV).contiguous(), rank.to(DEV), g_z.to(DEV), T.to(DEV)
    _hip.call("gs_z_backward", _hip.ptr(d_rank), _hip.ptr(d_gz), _hip.ptr(d_T), v_base, N, _hip.ptr(grad_xyz),
              _hip.current_stream())
    got = grad_xyz.cpu()
    assert torch.equal(got[culled], before[culled])           # culled rows: the same bits
    if N == 0:
        return
    vis = ~culled
    exact = before.double()[vis] + g_z.double()[(rank[vis] - v_base).long()][:, None] * T.double()[2, :3][None, :]
    err = (got.double()[vis] - exact).abs()
    # (1 + 1e-6: `exact` itself is a float64 sum, rounded at 1e-16)
    assert bool((err <= 2.0 ** -24 * (1 + 1e-6) * exact.abs() + 1e-45).all()), float((err / exact.abs().clamp(min=1e-300)).max())
    assert bool((got[vis] != before[vis]).any())


# ---- 3. the frame -----------------------------------------------------------------------------------------------------
BG = FRAME["bg"]


def frame_inputs(shift, grads=True):
    c = FRAME
    g, cam, T = make_scene(c["N"], c["W"], c["H"], 0, seed=c["seed"], device=DEV)
    g.opacity.add_(shift)
    if grads:
        for k in PARAMS:
            if getattr(g, k) is not None:
                getattr(g, k).requires_grad_(True)
    return g, cam, T, torch.full((3,), BG, device=DEV)


@functools.lru_cache(maxsize=None)
def frame_case(shift):
    """the frame's own uv / conic / opacity / xyz_camera_frame and complete lists (a return_aux frame), the depth
    reference on them for a seeded (g_depth, g_alpha), its unscaled-only twin and rule (a)'s bounds; once per shift"""
    g, cam, T, bg = frame_inputs(shift, grads=False)
    W, H = FRAME["W"], FRAME["H"]
    image, mask, uv, aux = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, return_aux=True, **DEFAULTS)
    cpu = lambda x: x.detach().cpu().contiguous()
    V = uv.shape[0]
    gen = torch.Generator().manual_seed(FRAME["seed"] + 2)
    base = SimpleNamespace(name=f"frame{shift}", W=W, H=H, V=V, uv=cpu(uv), conic=cpu(aux["conic"]),
                           opacity=cpu(aux["opacity"]).reshape(V, 1), rays=torch.zeros(H, W, 3),
                           sorted_g=cpu(aux["sorted_gaussians"]).int(), ranges=cpu(aux["tile_ranges"]).int())
    sc = D.as_depth_scene(base, cpu(aux["xyz_camera_frame"])[:, 2], torch.randn(H, W, 3, generator=gen))
    ref = D.reference_of(sc, sc.grad_image)
    scaled = ref.scale != 1
    true = D.reference_of(sc, sc.grad_image * (~scaled)[:, :, None]) if bool(scaled.any()) else ref
    vals = {}
    orc, bounds = oracle_bounds(vals, sc, true)
    return SimpleNamespace(sc=sc, ref=ref, true=true, orc=orc, bounds=bounds, vals=vals, image=cpu(image), mask=cpu(mask),
                           uv=cpu(uv))


def slab_fields(slab, g_z):
    return dict(g_z=g_z, g_opacity=slab[:, fused.SLAB_OPACITY], g_uv=slab[:, fused.SLAB_UV],
                g_conic=slab[:, fused.SLAB_CONIC])


def rgbd(g, T, cam, bg):
    return fused.rasterize_rgbd(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)


def fp32_fma_close(got, base, term):
    """got == base + term up to one fp32 rounding of the multiply-add (base fp32, term fp64)"""
    exact = base.double().cpu() + term.double().cpu()
    return bool(((got.double().cpu() - exact).abs() <= 2.0 ** -24 * (1 + 1e-6) * exact.abs() + 1e-45).all())


@pytest.mark.parametrize("shift", [FRAME["shift"], 0.0])
def test_frame_outputs_and_slab(shift):
    """fused.rasterize_rgbd on the 70 x 45 frame (shift -5.5: lists to 4186, the prefix repair runs; shift 0: pixels
    saturate, num_splats < list length): image / culling_mask / uv equal to fused.rasterize, depth / alpha by the
    forward rule, and with a loss on all three outputs the kept slab and last_grad_z() against the reference (the
    combined-slab rule of the module docstring; the colour part's reference is tests/test_gpu_render_ref64.py's),
    then the parameter gradients against fused.preprocess_backward on the kept slab"""
    case = frame_case(shift)
    sc, ref = case.sc, case.ref
    W, H = sc.W, sc.H
    if shift == FRAME["shift"]:
        assert R.max_list(sc) > 2 * 1024 and int(ref.nsp.max()) > 2 * 1024
    else:
        assert int(ref.nsp.max()) < R.max_list(sc) and float((ref.nsp < 600).float().mean()) > 0.5
    # the colour part of the combined slab: reference, oracle and grad_image of tests/test_gpu_render_ref64.py
    if shift == FRAME["shift"]:
        csc, cref, corc = frame_reference()
        assert torch.equal(csc.uv, sc.uv) and torch.equal(csc.sorted_g, sc.sorted_g)
        gi_image = cref.grad_image.float()
    else:
        cref, gi_image = None, None
    g, cam, T, bg = frame_inputs(shift)
    fused.keep_last_slab(True)
    try:
        fused.last_flags(clear=True)
        _hip.set_backward_mode("exact")
        image, depth, alpha, mask, uv = rgbd(g, T, cam, bg)
        flags = fused.last_flags()
        gd, ga = (ref.grad_image[..., i].float().to(DEV) for i in (0, 1))
        outs, gos = [depth, alpha], [gd, ga]
        if gi_image is not None:
            outs, gos = outs + [image], gos + [gi_image.to(DEV)]
        else:   # (a loss on all three outputs; no colour reference at this shift: the image's weight is zero)
            outs, gos = outs + [image], gos + [torch.zeros(H, W, 3, device=DEV)]
        torch.autograd.backward(outs, gos)
        slab, g_z = fused.last_slab(), fused.last_grad_z()
    finally:
        _hip.set_backward_mode("compat")
        fused.keep_last_slab(False)
    assert torch.equal(image.detach().cpu(), case.image) and torch.equal(mask.cpu(), case.mask)
    assert torch.equal(uv.detach().cpu(), case.uv)
    if shift == FRAME["shift"]:   # tiles ran out of the ordered prefix and were repaired
        assert flags is not None and int(flags.sum()) > 0
    assert tuple(depth.shape) == (H, W) and tuple(alpha.shape) == (H, W)
    assert slab is not None and g_z is not None and tuple(slab.shape) == (sc.V, 9) and tuple(g_z.shape) == (sc.V,)
    ok = ~ref.fragile
    vals = dict(case.vals, V=sc.V, max_list=R.max_list(sc), fragile=float(ref.fragile.float().mean()),
                scaled_pixels=float((ref.scale != 1).float().mean()))
    got = dict(depth=depth.detach().cpu(), alpha=alpha.detach().cpu())
    vals.update(forward_measures(got, case.orc, ref, ok))
    gslab = slab_fields(slab.cpu(), g_z.cpu())
    bounds = dict(case.bounds)
    want = SimpleNamespace(grad=dict(ref.grad), abs=dict(ref.abs), used=ref.used.clone())
    if cref is not None:
        for k in ("g_opacity", "g_uv", "g_conic"):
            want.grad[k] = ref.grad[k] + cref.grad_walk[k]
            want.abs[k] = ref.abs[k] + cref.abs_walk[k]
            b_c = D.noise_measure(corc[k], cref.grad_walk[k], cref.abs_walk[k]) + NOISE_MARGIN
            vals[f"colour_bound_{k}"] = b_c
            bounds[k] = max(bounds[k], b_c)
        want.used |= cref.used
    verdict = check_rule(vals, "b", gslab, want, bounds)
    report(f"depth_alpha_frame[shift {shift}]", **vals)
    assert vals["r_depth"] <= R_MAX and vals["r_alpha"] <= R_MAX, vals
    verdict()
    # the per-Gaussian node: the kept slab through fused.preprocess_backward on a fresh record, plus the z term
    g2, cam2, T2, _ = frame_inputs(shift, grads=False)
    f = fused.preprocess_forward(g2.xyz, g2.quaternion, g2.scale, g2.opacity, g2.rgb, g2.sh, T2, cam2.K, W, H,
                                 DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"],
                                 DEFAULTS["mh_dist"], None, 0)
    assert f.V == sc.V
    gx, gq, gs, go, gc, gsh = fused.preprocess_backward(g2.xyz, g2.quaternion, g2.scale, T2, cam2.K, f, slab.contiguous())
    for k, w in (("quaternion", gq), ("scale", gs), ("opacity", go), ("rgb", gc), ("sh", gsh)):
        if getattr(g, k) is not None:
            assert torch.equal(getattr(g, k).grad, w), k
    rank = f.rank.cpu().long()
    z_term = torch.zeros(FRAME["N"], 3, dtype=torch.float64)
    vis = rank >= 0
    z_term[vis] = g_z.double().cpu()[rank[vis]][:, None] * T2.double().cpu()[2, :3][None, :]
    assert fp32_fma_close(g.xyz.grad, gx, z_term)
    assert bool((g.xyz.grad.cpu()[vis] != gx.cpu()[vis]).any())


def param_grads(g):
    return {k: getattr(g, k).grad.clone() for k in PARAMS if getattr(g, k) is not None}


def calls_of(fn):
    _hip.enable_timing(True)
    try:
        fn()
        return _hip.collect_timing()
    finally:
        _hip.enable_timing(False)


@pytest.mark.parametrize("shift", [FRAME["shift"], 0.0])
def test_frame_subsets_of_the_outputs(shift):
    """a loss on the image alone: the parameter gradients of fused.rasterize (another order of the atomics, nothing
    else); a loss on alpha alone and on depth alone: finite, non-zero gradients and no colour backward; the unused
    outputs cost no launch"""
    w = torch.randn(FRAME["H"], FRAME["W"], 3, generator=torch.Generator().manual_seed(12)).to(DEV)
    g, cam, T, bg = frame_inputs(shift)
    image, mask, uv = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
    (image * w).sum().backward()
    want = param_grads(g)
    g, cam, T, bg = frame_inputs(shift)
    out = {}
    calls = calls_of(lambda: out.update(zip(("image", "depth", "alpha", "mask", "uv"), rgbd(g, T, cam, bg)))
                     or (out["image"] * w).sum().backward())
    assert torch.equal(out["image"].detach(), image.detach())
    assert "gs_render_zalpha_backward" not in calls and "gs_z_backward" not in calls
    assert len(calls["gs_render_zalpha"]) == 1 and len(calls["gs_render_tiles_backward_slab"]) == 1
    vals = {}
    for k, a in param_grads(g).items():
        vals[k] = rel_err(a, want[k])
        assert vals[k] < 1e-4, (k, vals[k])
    report(f"depth_alpha_frame_image_only[shift {shift}]", **vals)
    for which in ("alpha", "depth"):
        g, cam, T, bg = frame_inputs(shift)
        calls = calls_of(lambda: rgbd(g, T, cam, bg)[1 if which == "depth" else 2].sum().backward())
        assert "gs_render_tiles_backward_slab" not in calls, which
        assert len(calls["gs_render_backward_prologue"]) == 1 and len(calls["gs_render_zalpha_backward"]) == 1
        assert len(calls.get("gs_z_backward", [])) == (1 if which == "depth" else 0)
        for k, a in param_grads(g).items():
            assert bool(torch.isfinite(a).all()), (which, k)
            assert (k == "rgb") != bool(a.any()), (which, k)     # the colour has no part in depth or alpha


def test_frame_with_nothing_visible():
    g, cam, T, bg = frame_inputs(0.0)
    T.requires_grad_(True)
    image, depth, alpha, mask, uv = fused.rasterize_rgbd(g, T, cam, 0.1, 0.2, 100, 3.0, True, bg)
    assert uv.shape[0] == 0 and bool(mask.all())
    assert tuple(depth.shape) == (FRAME["H"], FRAME["W"]) and not depth.any() and not alpha.any()
    assert bool((image == BG).all())
    (depth.sum() + alpha.sum() + image.sum()).backward()
    for k, a in param_grads(g).items():
        assert not a.any(), k
    assert T.grad is None or not T.grad.any()


# ---- 4. the pose ------------------------------------------------------------------------------------------------------
def test_pose_gradient_of_a_depth_loss():
    """517 x 301, 3000 Gaussians, camera_T_world requires grad, loss on depth alone: T.grad against the closed form
    of tests/pose_terms.py on the kept slab plus the float64 sum of the direct term of z = T[2, 0:3] . xyz + T[2, 3]
    on the kept g_z (dL/dT[2, 0:3] += sum g_z xyz, dL/dT[2, 3] += sum g_z); pose_r with the z term's |t64| and
    |t32 - t64| added to B and E"""
    sc = general_camera_scene(90, 3000, deg=1, kind="odd", stress=True)
    g, cam, T = to_device(sc, DEV)
    for k in PARAMS:
        getattr(g, k).requires_grad_(True)
    T.requires_grad_(True)
    bg = torch.full((3,), 0.5, device=DEV)
    w = torch.randn(sc.H, sc.W, generator=torch.Generator().manual_seed(4)).to(DEV) / (sc.W * sc.H)
    fused.keep_last_slab(True)
    try:
        image, depth, alpha, mask, uv = fused.rasterize_rgbd(g, T, cam, sc.near, sc.far, sc.pad, sc.mh, True, bg)
        (depth * w).sum().backward()
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
    share = float((t64.sum(0).abs()[2] / ref.abs()[2].clamp(min=1e-300)).max())
    report("depth_alpha_pose[depth loss]", r=r, z_term_share=share)
    print(f"depth_alpha_pose: r = {r:.3g}, direct z term / total (row 2) up to {share:.3g}")
    assert r <= R_MAX, r
    assert bool(t64.sum(0)[2].abs().max() > 0)


# ---- 5. the guards ----------------------------------------------------------------------------------------------------
def test_guards_raise_and_leave_the_next_frame_alone():
    case = frame_case(0.0)
    g, cam, T, bg = frame_inputs(0.0, grads=False)
    args = (g, T, cam, DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"], DEFAULTS["mh_dist"])
    sh = torch.zeros(FRAME["N"], 3, 3, device=DEV)
    g_sh = type(g)(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, sh)
    cpu = lambda x: None if x is None else x.cpu()
    g_cpu = type(g)(cpu(g.xyz), cpu(g.rgb), cpu(g.opacity), cpu(g.scale), cpu(g.quaternion), None)
    g_f64 = type(g)(g.xyz.double(), g.rgb.double(), g.opacity.double(), g.scale.double(), g.quaternion.double(), None)
    bad = [
        ("tile_rows", lambda: fused.rasterize_rgbd(*args, True, bg, tile_rows=(0, 2))),
        ("return_aux", lambda: fused.rasterize_rgbd(*args, True, bg, return_aux=True)),
        ("slab_sync", lambda: fused.rasterize_rgbd(*args, True, bg, slab_sync=lambda flat: None)),
        ("grad_sync", lambda: fused.rasterize_rgbd(*args, True, bg, grad_sync=lambda t: None)),
        ("frame_hook", lambda: fused.rasterize_rgbd(*args, True, bg, frame_hook=lambda d: None)),
        ("adam_plan", lambda: fused.rasterize_rgbd(*args, True, bg, adam_plan=object())),
        ("per-pixel SH", lambda: fused.rasterize_rgbd(g_sh, *args[1:], False, bg)),
        ("CPU", lambda: fused.rasterize_rgbd(g_cpu, cpu(T), type(cam)(cam.width, cam.height, cpu(cam.K)), *args[3:], True,
                                             cpu(bg))),
        ("float", lambda: fused.rasterize_rgbd(g_f64, T.double(), type(cam)(cam.width, cam.height, cam.K.double()),
                                               *args[3:], True, bg.double())),
    ]
    for words, call in bad:
        with pytest.raises(RuntimeError, match=words):
            call()
        image, depth, alpha, mask, uv = fused.rasterize_rgbd(*args, True, bg)
        assert torch.equal(image.cpu(), case.image) and torch.equal(uv.cpu(), case.uv), words
        m = forward_measures(dict(depth=depth.cpu(), alpha=alpha.cpu()), case.orc, case.ref, ~case.ref.fragile)
        assert m["r_depth"] <= R_MAX and m["r_alpha"] <= R_MAX, (words, m)
    # SH with the precompute mode is supported
    image, depth, alpha, mask, uv = fused.rasterize_rgbd(g_sh, *args[1:], True, bg)
    assert bool(torch.isfinite(image).all()) and bool(torch.isfinite(depth).all())
