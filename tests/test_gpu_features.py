"""Per-Gaussian feature maps: gs_render_features / gs_render_features_backward and fused.rasterize_features against
tests/render_ref64.py fed the feature channels as colours, three per call (tests/features_ref.py; the inputs are held
to what this file needs by tests/test_features_ref.py on the CPU).

Rules (the measures and bounds of tests/test_gpu_depth_alpha.py, imported, unchanged):
  forward    on the non-fragile pixels, ref64.r_measure of every channel of feature_map and of alpha with
             env = |fp32 oracle - reference| <= R_MAX
  (a)        gradients only on the pixels whose reference walk is not scaled (scale == 1), where the fp32 oracle's
             gradient is the true derivative: noise_measure of the kernel per tensor (g_features, g_opacity, g_uv,
             g_conic) <= the oracle's + NOISE_MARGIN
  (b)        all non-fragile pixels against the TRUE derivative `grad`: the same number as (a)'s bound for that scene,
             channel count and tensor
  a slab that also holds the colour backward's gradient (the frame test, loss on all three outputs): the measure
             against ref = grad_walk(colour) + grad(features), abs = abs_c + abs_f is held to max(B_c, B_f), as the
             depth test's combined slab
  bit-equalities: alpha and transmittance of gs_render_zalpha; with one channel holding z its depth

One rule is not the depth file's.  NULL = zeros is bit-equal on a one-tile scene for the slab (one atomic per value per
(entry, tile)); grad_features receives one atomic per value per (entry, 8 x 8 patch) by design, up to four per row on
one tile in whatever order the waves arrive, so there two runs agree to 3 x 2^-24 of the terms' magnitudes (PATCH_SUMS)
and to the bit once the gradient is confined to one patch (test_null_gradients_are_zeros).

Measured on an MI355X (every case leaves its figures in the parity report):
  kernels, 26 cases       r_feature_map 0.58 to 4.45 (long_1100, C = 17), r_alpha 0.37 to 2.11 (long_1100); fragile 0 %,
                          scaled pixels 0 to 57 %
             rule (a)     kernel 6.7e-6 at most (long_1100, g_features; oracle 6.5e-6), 9.5e-7 at most on the other
                          scenes; opaque_stack: kernel 3.0e-7 where the oracle, which starts from 1 - A, has 3.3e-4
             rule (b)     kernel 4.4e-6 at most (long_1100, g_features), 9.6e-7 elsewhere
  NULL = zeros            slab tensors equal to the bit on both scenes; g_features within 1.9e-8 (four patch sums)
  frame, shift -5.5       r_feature_map 2.3, r_alpha 2.1; combined slab 5.3e-6 (g_opacity) against bounds of 3.3e-5 to
                          3.6e-5, g_features 2.0e-6 against 3.3e-5; 96 % of the pixels scaled; no Gaussian culled
  frame, shift 0          r_feature_map 1.1, r_alpha 1.7; slab and g_features 1.4e-6 at most (oracle: 8.3e-4)
  image-only loss         parameter gradients within 6.6e-6 (rel_err) of fused.rasterize's
  pose, feature loss      r 0.41 to 0.45"""
import functools
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS

from . import depth_alpha_ref as D
from . import features_ref as F
from . import render_ref64 as R
from .helpers import rel_err, report
from .pose_terms import pose_r, pose_reference
from .ref64 import general_camera_scene, to_device
from .test_gpu_depth_alpha import (BG, FRAME, NOISE_MARGIN, PARAMS, R_MAX, calls_of, frame_inputs, frame_reference,
                                   param_grads, r_measure)
from .test_render_ref64 import oracle_run

noise_measure = D.noise_measure   # (tests/test_gpu_render_ref64.py's, as the depth tests take it)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCENES = list(R.render_scenes())
SENTINEL = -777.0
SLACK = 32   # floats behind feature_map / grad_features: a whole padded row of the widest instantiation
# every count at which another instantiation (4, 8, 16, 32) runs: each largest count and one past a boundary
COUNTS = (1, 3, 4, 5, 16, 17, 32)
KERNEL_CASES = [(name, C) for name in SCENES for C in (5, 32)] + \
               [(name, C) for name in ("partial_33x17", "long_1100") for C in COUNTS if C not in (5, 32)]


# ---- 1. the kernels against the reference -----------------------------------------------------------------------------
def kernel_run(sc, feat, g_map, g_alpha, pattern=None, want_gf=True, rows=None):
    """scene sc with feature rows feat [V, C] through gs_pack_splats, gs_render_tiles_packed (for
    num_splats_per_pixel), gs_render_features and gs_render_features_backward -> dict of CPU tensors.
    g_map [H, W, C] / g_alpha [H, W] or None (NULL); pattern [V, 3]: what the slab's columns 0..2 hold before the call;
    want_gf False: grad_features is NULL; rows: (tile_row0, tile_row1) of both calls.  feature_map and grad_features
    lie in buffers with SLACK floats behind them, pre-filled with SENTINEL (feature_map: all of it)."""
    c = lambda x: x.to(DEV).float().contiguous() if x.is_floating_point() else x.to(DEV).contiguous()
    V, W, H, C = sc.V, sc.W, sc.H, int(feat.shape[1])
    nty = (H + 15) // 16
    row0, row1 = rows if rows is not None else (0, nty)
    s = _hip.current_stream()
    p = _hip.ptr
    uv, opacity, conic, rgb = c(sc.uv), c(sc.opacity), c(sc.conic), torch.zeros(V, 3, device=DEV)
    ranges, sorted_g, bg = c(sc.ranges), c(sc.sorted_g), torch.zeros(3, device=DEV)
    packed = torch.empty(V, 12, device=DEV)
    _hip.call("gs_pack_splats", p(uv), p(opacity), p(conic), p(rgb), V, p(packed), _hip.GS_F32, s)
    image = torch.zeros(H, W, 3, device=DEV)
    fw = torch.zeros(H, W, device=DEV)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    _hip.call("gs_render_tiles_packed", p(packed), p(rgb), None, p(ranges), p(sorted_g), p(bg), W, H, 1, 0, nty, p(nsp),
              p(fw), p(image), _hip.GS_F32, None, s)
    d_feat = c(feat)
    fbuf = torch.full((H * W * C + SLACK,), SENTINEL, device=DEV)
    fmap = fbuf[:H * W * C].view(H, W, C)
    alpha, t_end = (torch.full((H, W), SENTINEL, device=DEV) for _ in range(2))
    _hip.call("gs_render_features", p(packed), p(d_feat), C, p(ranges), p(sorted_g), p(nsp), W, H, row0, row1, p(fmap),
              p(alpha), p(t_end), s)
    slab = torch.zeros(V, 9, device=DEV)
    if pattern is not None:
        slab[:, :3] = pattern.to(DEV)
    gbuf = torch.cat([torch.zeros(V * C, device=DEV), torch.full((SLACK,), SENTINEL, device=DEV)])
    gf = gbuf[:V * C].view(V, C)
    gm = None if g_map is None else c(g_map)
    ga = None if g_alpha is None else c(g_alpha)
    if rows is None or row1 > row0:
        t_in = t_end if rows is None else torch.where(t_end == SENTINEL, torch.ones_like(t_end), t_end)
        _hip.call("gs_render_features_backward", p(packed), p(d_feat), C, p(ranges), p(sorted_g), p(nsp), p(t_in), p(gm),
                  p(ga), W, H, row0, row1, p(slab), p(gf) if want_gf else None, s)
    slab = slab.cpu()
    return dict(nsp=nsp.cpu(), feature_map=fmap.cpu(), alpha=alpha.cpu(), t_end=t_end.cpu(), colour=slab[:, :3],
                g_features=gf.cpu(), g_opacity=slab[:, fused.SLAB_OPACITY], g_uv=slab[:, fused.SLAB_UV],
                g_conic=slab[:, fused.SLAB_CONIC], map_slack=fbuf[H * W * C:].cpu(), grad_slack=gbuf[V * C:].cpu())


def forward_measures(got, orc, ref, ok):
    n = int(ok.sum())
    pick = lambda x: x.double()[ok].reshape(n, -1)
    return {f"r_{k}": r_measure(pick(got[k]), pick(getattr(ref, k)), pick(orc[k]) - pick(getattr(ref, k)))
            for k in ("feature_map", "alpha")}


def oracle_bounds(vals, sc, true):
    """rule (a)'s right-hand side per tensor: the fp32 oracle's measure on the unscaled pixels + NOISE_MARGIN"""
    orc = F.oracle_of(sc, true.grad_image.float(), oracle_run)
    for k in F.KEYS:
        vals[f"a_oracle_{k}"] = noise_measure(orc[k], true.grad[k], true.abs[k])
    return orc, {k: vals[f"a_oracle_{k}"] + NOISE_MARGIN for k in F.KEYS}


def check_rule(vals, tag, got, want, bounds, keys=F.KEYS):
    for k in keys:
        vals[f"{tag}_kernel_{k}"] = noise_measure(got[k], want.grad[k], want.abs[k])

    def verdict():
        for k in keys:
            assert vals[f"{tag}_kernel_{k}"] <= bounds[k], (tag, k, vals)
            assert not got[k][~want.used].any(), (tag, k)         # rows no pixel uses: exactly zero
            assert got[k][want.used].abs().max() > 0, (tag, k)
    return verdict


@pytest.mark.parametrize("name,C", KERNEL_CASES)
def test_kernels_against_the_reference(name, C):
    sc = F.features_scene(name, C)
    ref, true = F.reference(name, C), F.reference(name, C, True)
    ok = ~ref.fragile
    vals = {"scaled_pixels": float((ref.scale != 1).float().mean()), "fragile": float(ref.fragile.float().mean())}
    orc, bounds = oracle_bounds(vals, sc, true)
    pattern = torch.randn(sc.V, 3, generator=torch.Generator().manual_seed(3))
    runs = {}
    for tag, r in (("a", true), ("b", ref)):
        gi = r.grad_image.float()
        runs[tag] = kernel_run(sc, sc.feat, gi[..., :C], gi[..., C], pattern)
        assert torch.equal(runs[tag]["colour"], pattern), tag         # the slab's columns 0..2 as they were
        # nothing beyond column C - 1 of the last row is written, whatever the padded instantiation
        assert bool((runs[tag]["map_slack"] == SENTINEL).all()) and bool((runs[tag]["grad_slack"] == SENTINEL).all()), tag
    got = runs["b"]
    assert torch.equal(got["nsp"][ok], ref.nsp[ok])
    for k in ("feature_map", "alpha", "t_end"):
        assert bool(torch.isfinite(got[k]).all()) and not bool((got[k] == SENTINEL).any()), k   # every pixel is written
    vals.update(forward_measures(got, orc, ref, ok))
    verdicts = [check_rule(vals, "a", runs["a"], true, bounds), check_rule(vals, "b", runs["b"], ref, bounds)]
    report(f"features_kernels[{name}, C={C}]", **vals)
    assert vals["r_feature_map"] <= R_MAX and vals["r_alpha"] <= R_MAX, vals
    for v in verdicts:
        v()


# ---- 2. bit-equalities with the depth kernels -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["partial_48x40", "long_1100"])
def test_bit_equal_to_the_depth_kernels(name):
    from .test_gpu_depth_alpha import kernel_run as depth_run
    dsc = D.depth_scene(name)
    zero = torch.zeros(dsc.H, dsc.W)
    want = depth_run(dsc, zero, zero)
    got = kernel_run(dsc, dsc.z.reshape(-1, 1), None, zero)
    assert torch.equal(got["nsp"], want["nsp"])
    assert torch.equal(got["alpha"], want["alpha"]) and torch.equal(got["t_end"], want["t_end"])
    assert torch.equal(got["feature_map"][..., 0], want["depth"])
    assert float(want["depth"].abs().max()) > 0
    # and with more channels: alpha and the transmittance do not depend on the features
    fsc = F.features_scene(name, 5)
    got5 = kernel_run(fsc, fsc.feat, None, zero)
    assert torch.equal(got5["alpha"], want["alpha"]) and torch.equal(got5["t_end"], want["t_end"])


# ---- 3. NULL handling and validation ----------------------------------------------------------------------------------
PATCH_SUMS = 3 * 2.0 ** -24   # four addends in any order: at most three roundings of at most 2^-24 of the terms' sum


@pytest.mark.parametrize("name", ["partial_33x17", "opaque_stack"])
def test_null_gradients_are_zeros(name):
    """NULL grad_feature_map or grad_alpha = zeros.  The slab: one atomic per value per (entry, tile), so on a one-tile
    scene the same bits, on several tiles the sums of a row arrive in another order (noise_measure <= 1e-6 as in the
    depth test).  grad_features gets one atomic per value per (entry, 8 x 8 patch): a one-tile scene adds up to four
    patch sums into a row in whatever order the waves arrive, so two runs of the same call agree to PATCH_SUMS of the
    terms' magnitudes, not to the bit -- and to the bit once the gradient is confined to one patch, where the other
    three add exact zeros.  NULL grad_features leaves the slab's result as it is."""
    C = 5
    sc, ref = F.features_scene(name, C), F.reference(name, C)
    gi = ref.grad_image.float()
    gm, ga = gi[..., :C].contiguous(), gi[..., C].contiguous()
    one_tile = sc.ranges.numel() == 2
    vals = {}

    def same(a, b, keys, what, one_patch=False):
        for k in keys:
            vals[f"{what}_{k}"] = noise_measure(a[k], b[k], ref.abs[k])
            if one_tile and (k != "g_features" or one_patch):
                assert torch.equal(a[k], b[k]), (what, k)
            else:
                assert vals[f"{what}_{k}"] <= (PATCH_SUMS if one_tile else 1e-6), (what, k, vals)

    a, b = kernel_run(sc, sc.feat, None, ga), kernel_run(sc, sc.feat, torch.zeros_like(gm), ga)
    same(a, b, F.KEYS, "map")
    assert not a["g_features"].any() and not b["g_features"].any() and a["g_opacity"].abs().max() > 0
    a, b = kernel_run(sc, sc.feat, gm, None), kernel_run(sc, sc.feat, gm, torch.zeros_like(ga))
    same(a, b, F.KEYS, "alpha")
    assert a["g_features"].abs().max() > 0 and a["g_opacity"].abs().max() > 0
    # the gradient confined to the first 8 x 8 patch of the first tile
    gm1 = torch.zeros_like(gm)
    gm1[:8, :8] = gm[:8, :8]
    a, b = kernel_run(sc, sc.feat, gm1, None), kernel_run(sc, sc.feat, gm1, torch.zeros_like(ga))
    same(a, b, F.KEYS, "alpha_one_patch", one_patch=True)
    assert a["g_features"].abs().max() > 0
    a, b = kernel_run(sc, sc.feat, gm, ga, want_gf=False), kernel_run(sc, sc.feat, gm, ga)
    same(a, b, F.SHARED, "grad_features")
    assert not a["g_features"].any() and bool((a["grad_slack"] == SENTINEL).all())
    # both NULL: nothing is added anywhere
    a = kernel_run(sc, sc.feat, None, None)
    for k in F.KEYS:
        assert not a[k].any(), k
    report(f"features_null[{name}]", **vals)


def test_kernel_entry_points_validate():
    """bad arguments are GS_EINVAL with a message; both gradients NULL, zero tile rows, V == 0 and empty lists launch
    nothing harmful; tile rows write only their rows"""
    lib, s = _hip.lib(), _hip.current_stream()
    p = _hip.ptr
    z = torch.zeros(4, device=DEV)
    assert lib.gs_render_features(None, None, 4, None, None, None, 0, 16, 0, 1, p(z), p(z), p(z), s) == _hip.GS_EINVAL
    assert b"non-empty" in lib.gs_last_error()
    assert lib.gs_render_features(None, None, 4, p(z), None, p(z), 16, 16, 0, 2, p(z), p(z), p(z), s) == _hip.GS_EINVAL
    assert b"tile row" in lib.gs_last_error()
    for bad in (0, 33, -1):
        assert lib.gs_render_features(None, None, bad, p(z), None, p(z), 16, 16, 0, 1, p(z), p(z), p(z), s) == _hip.GS_EINVAL
        assert b"1..32" in lib.gs_last_error()
        assert lib.gs_render_features_backward(None, None, bad, p(z), None, p(z), p(z), p(z), p(z), 16, 16, 0, 1, p(z),
                                               p(z), s) == _hip.GS_EINVAL
        assert b"1..32" in lib.gs_last_error()
    assert lib.gs_render_features_backward(None, None, 4, p(z), None, p(z), None, None, None, 16, 16, 0, 1, None, None,
                                           s) == _hip.GS_EINVAL
    assert lib.gs_render_features_backward(None, None, 4, p(z), None, p(z), p(z), p(z), None, 16, 16, 0, 1, None, None,
                                           s) == _hip.GS_EINVAL
    assert b"grad_slab" in lib.gs_last_error()
    # empty lists, V == 0: zeros and a transmittance of one; the backward adds nothing
    W, H, C = 33, 17, 5
    ranges = torch.zeros(3 * 2 + 1, dtype=torch.int32, device=DEV)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    fm = torch.full((H, W, C), 7.0, device=DEV)
    a, t = (torch.full((H, W), 7.0, device=DEV) for _ in range(2))
    e = torch.empty(0, device=DEV)
    _hip.call("gs_render_features", p(e), p(e), C, p(ranges), p(e), p(nsp), W, H, 0, 2, p(fm), p(a), p(t), s)
    assert not fm.any() and not a.any() and bool((t == 1).all())
    slab, gf = torch.ones(1, 9, device=DEV), torch.ones(1, C, device=DEV)
    ones = torch.ones(H, W, C, device=DEV)
    _hip.call("gs_render_features_backward", p(e), p(e), C, p(ranges), p(e), p(nsp), p(t), p(ones), p(a), W, H, 0, 2,
              p(slab), p(gf), s)
    _hip.call("gs_render_features_backward", p(e), p(e), C, p(ranges), p(e), p(nsp), p(t), None, None, W, H, 0, 2, None,
              None, s)
    # zero tile rows
    _hip.call("gs_render_features", p(e), p(e), C, p(ranges), p(e), p(nsp), W, H, 1, 1, p(fm), p(a), p(t), s)
    _hip.call("gs_render_features_backward", p(e), p(e), C, p(ranges), p(e), p(nsp), p(t), p(ones), p(a), W, H, 1, 1,
              p(slab), p(gf), s)
    torch.cuda.synchronize()
    assert bool((slab == 1).all()) and bool((gf == 1).all())
    # tile rows: only the rows asked for are written, and only their pixels' gradients are added
    sc, ref = F.features_scene("partial_33x17", C), F.reference("partial_33x17", C)
    gi = ref.grad_image.float()
    gm, ga = gi[..., :C].contiguous(), gi[..., C].contiguous()
    whole, part = kernel_run(sc, sc.feat, gm, ga), kernel_run(sc, sc.feat, gm, ga, rows=(1, 2))
    for k in ("feature_map", "alpha", "t_end"):
        assert bool((part[k][:16] == SENTINEL).all()) and torch.equal(part[k][16:], whole[k][16:]), k
    below = gm.clone()
    below[:16] = 0
    ga_below = ga.clone()
    ga_below[:16] = 0
    want = kernel_run(sc, sc.feat, below, ga_below)
    for k in F.KEYS:
        assert noise_measure(part[k], want[k], ref.abs[k]) <= 1e-6, k
    assert part["g_opacity"].abs().max() > 0


# ---- 4. the frame -----------------------------------------------------------------------------------------------------
C_FRAME = 5


def frame_features(grad=True):
    gen = torch.Generator().manual_seed(FRAME["seed"] + 3)
    return torch.randn(FRAME["N"], C_FRAME, generator=gen).to(DEV).requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def frame_case(shift):
    """the frame's own uv / conic / opacity and complete lists (a return_aux frame), the features reference on them for
    a seeded [g_F | g_alpha], its unscaled-only twin and rule (a)'s bounds; once per shift"""
    g, cam, T, bg = frame_inputs(shift, grads=False)
    W, H = FRAME["W"], FRAME["H"]
    image, mask, uv, aux = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, return_aux=True, **DEFAULTS)
    cpu = lambda x: x.detach().cpu().contiguous()
    V = uv.shape[0]
    vis_idx = cpu(aux["vis_idx"]).long()[:V]
    gen = torch.Generator().manual_seed(FRAME["seed"] + 4)
    base = SimpleNamespace(name=f"frame{shift}", W=W, H=H, V=V, uv=cpu(uv), conic=cpu(aux["conic"]),
                           opacity=cpu(aux["opacity"]).reshape(V, 1), rays=torch.zeros(H, W, 3),
                           sorted_g=cpu(aux["sorted_gaussians"]).int(), ranges=cpu(aux["tile_ranges"]).int())
    sc = F.as_features_scene(base, frame_features(False).cpu()[vis_idx], torch.randn(H, W, C_FRAME + 1, generator=gen))
    ref = F.reference_of(sc, sc.g_all)
    scaled = ref.scale != 1
    true = F.reference_of(sc, sc.g_all * (~scaled)[:, :, None]) if bool(scaled.any()) else ref
    vals = {}
    orc, bounds = oracle_bounds(vals, sc, true)
    return SimpleNamespace(sc=sc, ref=ref, true=true, orc=orc, bounds=bounds, vals=vals, image=cpu(image), mask=cpu(mask),
                           uv=cpu(uv), vis_idx=vis_idx)


def feats(g, f, T, cam, bg):
    return fused.rasterize_features(g, f, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)


@pytest.mark.parametrize("shift", [FRAME["shift"], 0.0])
def test_frame_outputs_and_slab(shift):
    """fused.rasterize_features on the 70 x 45 frame (shift -5.5: lists beyond 2 x 1024, the prefix repair runs; shift
    0: pixels saturate) with C = 5: image / culling_mask / uv equal to fused.rasterize, feature_map / alpha by the
    forward rule, and with a loss on all three outputs the kept slab against grad_walk(colour) + grad(features) (the
    combined-slab rule), features.grad against the reference through vis_idx with culled rows exactly zero, then the
    parameter gradients against fused.preprocess_backward on the kept slab"""
    case = frame_case(shift)
    sc, ref = case.sc, case.ref
    W, H, C = sc.W, sc.H, C_FRAME
    if shift == FRAME["shift"]:
        assert R.max_list(sc) > 2 * 1024 and int(ref.nsp.max()) > 2 * 1024
        csc, cref, corc = frame_reference()
        assert torch.equal(csc.uv, sc.uv) and torch.equal(csc.sorted_g, sc.sorted_g)
        gi_image = cref.grad_image.float()
    else:
        assert int(ref.nsp.max()) < R.max_list(sc) and float((ref.nsp < 600).float().mean()) > 0.5
        cref, gi_image = None, torch.zeros(H, W, 3)   # (no colour reference at this shift: the image's weight is zero)
    g, cam, T, bg = frame_inputs(shift)
    f = frame_features()
    fused.keep_last_slab(True)
    try:
        fused.last_flags(clear=True)
        _hip.set_backward_mode("exact")
        image, fmap, alpha, mask, uv = feats(g, f, T, cam, bg)
        flags = fused.last_flags()
        gi = ref.grad_image.float().to(DEV)
        torch.autograd.backward([fmap, alpha, image], [gi[..., :C].contiguous(), gi[..., C].contiguous(), gi_image.to(DEV)])
        slab = fused.last_slab()
    finally:
        _hip.set_backward_mode("compat")
        fused.keep_last_slab(False)
    assert torch.equal(image.detach().cpu(), case.image) and torch.equal(mask.cpu(), case.mask)
    assert torch.equal(uv.detach().cpu(), case.uv)
    if shift == FRAME["shift"]:   # tiles ran out of the ordered prefix and were repaired
        assert flags is not None and int(flags.sum()) > 0
    assert tuple(fmap.shape) == (H, W, C) and tuple(alpha.shape) == (H, W)
    assert slab is not None and tuple(slab.shape) == (sc.V, 9)
    assert f.grad is not None and tuple(f.grad.shape) == (FRAME["N"], C)
    ok = ~ref.fragile
    vals = dict(case.vals, V=sc.V, max_list=R.max_list(sc), fragile=float(ref.fragile.float().mean()),
                scaled_pixels=float((ref.scale != 1).float().mean()))
    vals.update(forward_measures(dict(feature_map=fmap.detach().cpu(), alpha=alpha.detach().cpu()), case.orc, ref, ok))
    fg = f.grad.cpu()
    cs = slab.cpu()
    got = dict(g_features=fg[case.vis_idx], g_opacity=cs[:, fused.SLAB_OPACITY], g_uv=cs[:, fused.SLAB_UV],
               g_conic=cs[:, fused.SLAB_CONIC])
    bounds = dict(case.bounds)
    want = SimpleNamespace(grad=dict(ref.grad), abs=dict(ref.abs), used=ref.used.clone())
    want_f = SimpleNamespace(grad=ref.grad, abs=ref.abs, used=ref.used)
    verdict_f = check_rule(vals, "b", got, want_f, bounds, keys=("g_features",))   # (the colour has no part in it)
    if cref is not None:
        for k in F.SHARED:
            want.grad[k] = ref.grad[k] + cref.grad_walk[k]
            want.abs[k] = ref.abs[k] + cref.abs_walk[k]
            b_c = noise_measure(corc[k], cref.grad_walk[k], cref.abs_walk[k]) + NOISE_MARGIN
            vals[f"colour_bound_{k}"] = b_c
            bounds[k] = max(bounds[k], b_c)
        want.used = want.used | cref.used
    verdict = check_rule(vals, "b", got, want, bounds, keys=F.SHARED)
    report(f"features_frame[shift {shift}]", **vals)
    assert vals["r_feature_map"] <= R_MAX and vals["r_alpha"] <= R_MAX, vals
    verdict_f()
    verdict()
    culled = torch.ones(FRAME["N"], dtype=torch.bool)
    culled[case.vis_idx] = False
    assert not fg[culled].any()              # culled rows: exactly zero (this frame culls none; the test below does)
    # the per-Gaussian node: the kept slab through fused.preprocess_backward on a fresh record
    g2, cam2, T2, _ = frame_inputs(shift, grads=False)
    rec = fused.preprocess_forward(g2.xyz, g2.quaternion, g2.scale, g2.opacity, g2.rgb, g2.sh, T2, cam2.K, W, H,
                                   DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"],
                                   DEFAULTS["mh_dist"], None, 0)
    assert rec.V == sc.V
    gx, gq, gs, go, gc, gsh = fused.preprocess_backward(g2.xyz, g2.quaternion, g2.scale, T2, cam2.K, rec, slab.contiguous())
    for k, w in (("xyz", gx), ("quaternion", gq), ("scale", gs), ("opacity", go), ("rgb", gc), ("sh", gsh)):
        if getattr(g, k) is not None:
            assert torch.equal(getattr(g, k).grad, w), k


@pytest.mark.parametrize("shift", [FRAME["shift"], 0.0])
def test_frame_subsets_of_the_outputs(shift):
    """a loss on the image alone: the parameter gradients of fused.rasterize and no features backward; a loss on the
    feature map alone or alpha alone: no colour backward; features that require no gradient: the geometry still gets
    its own; the unused outputs cost no launch"""
    w = torch.randn(FRAME["H"], FRAME["W"], 3, generator=torch.Generator().manual_seed(12)).to(DEV)
    g, cam, T, bg = frame_inputs(shift)
    image, mask, uv = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
    (image * w).sum().backward()
    want = param_grads(g)
    g, cam, T, bg = frame_inputs(shift)
    f = frame_features()
    out = {}
    calls = calls_of(lambda: out.update(zip(("image", "fmap", "alpha", "mask", "uv"), feats(g, f, T, cam, bg)))
                     or (out["image"] * w).sum().backward())
    assert torch.equal(out["image"].detach(), image.detach())
    assert "gs_render_features_backward" not in calls
    assert len(calls["gs_render_features"]) == 1 and len(calls["gs_render_tiles_backward_slab"]) == 1
    assert f.grad is None or not f.grad.any()
    vals = {}
    for k, a in param_grads(g).items():
        vals[k] = rel_err(a, want[k])
        assert vals[k] < 1e-4, (k, vals[k])
    report(f"features_frame_image_only[shift {shift}]", **vals)
    wf = torch.randn(FRAME["H"], FRAME["W"], C_FRAME, generator=torch.Generator().manual_seed(13)).to(DEV)
    for which in ("alpha", "fmap", "fmap_const"):
        g, cam, T, bg = frame_inputs(shift)
        f = frame_features(grad=which != "fmap_const")
        loss = (lambda o: o[2].sum()) if which == "alpha" else (lambda o: (o[1] * wf).sum())
        calls = calls_of(lambda: loss(feats(g, f, T, cam, bg)).backward())
        assert "gs_render_tiles_backward_slab" not in calls, which
        assert len(calls["gs_render_backward_prologue"]) == 1 and len(calls["gs_render_features_backward"]) == 1
        for k, a in param_grads(g).items():
            assert bool(torch.isfinite(a).all()), (which, k)
            assert (k == "rgb") != bool(a.any()), (which, k)     # the colour has no part in the feature map or alpha
        if which == "fmap":
            assert bool(torch.isfinite(f.grad).all()) and bool(f.grad.any())
        elif which == "alpha":
            assert f.grad is None or not f.grad.any()
        else:
            assert f.grad is None


def test_frame_with_nothing_visible():
    g, cam, T, bg = frame_inputs(0.0)
    f = frame_features()
    T.requires_grad_(True)
    image, fmap, alpha, mask, uv = fused.rasterize_features(g, f, T, cam, 0.1, 0.2, 100, 3.0, True, bg)
    assert uv.shape[0] == 0 and bool(mask.all())
    assert tuple(fmap.shape) == (FRAME["H"], FRAME["W"], C_FRAME) and not fmap.any() and not alpha.any()
    assert bool((image == BG).all())
    (fmap.sum() + alpha.sum() + image.sum()).backward()
    for k, a in param_grads(g).items():
        assert not a.any(), k
    assert f.grad is None or not f.grad.any()
    assert T.grad is None or not T.grad.any()


def test_culled_rows_get_exactly_zero_feature_gradient():
    """the far plane at the median camera-frame z: half the Gaussians are culled, their rows of features.grad are
    exactly zero and those of the visible ones are not all zero"""
    g, cam, T, bg = frame_inputs(0.0)
    f = frame_features()
    z = (g.xyz.detach() @ T[2, :3] + T[2, 3])
    far = float(z.median())
    image, fmap, alpha, mask, uv = fused.rasterize_features(g, f, T, cam, DEFAULTS["near_thresh"], far,
                                                            DEFAULTS["cull_mask_padding"], DEFAULTS["mh_dist"], True, bg)
    w = torch.randn(FRAME["H"], FRAME["W"], C_FRAME, generator=torch.Generator().manual_seed(14)).to(DEV)
    (fmap * w).sum().backward()
    assert 0.25 * FRAME["N"] < int(mask.sum()) < 0.75 * FRAME["N"] and uv.shape[0] == int((~mask).sum())
    assert tuple(f.grad.shape) == (FRAME["N"], C_FRAME)
    assert not f.grad[mask].any() and bool(f.grad[~mask].any()) and bool(torch.isfinite(f.grad).all())


# ---- 5. the pose ------------------------------------------------------------------------------------------------------
def test_pose_gradient_of_a_feature_loss():
    """517 x 301, 3000 Gaussians, camera_T_world requires grad, loss on feature_map alone (C = 4): T.grad against the
    closed form of tests/pose_terms.py on the kept slab; features have no direct pose term"""
    sc = general_camera_scene(90, 3000, deg=1, kind="odd", stress=True)
    g, cam, T = to_device(sc, DEV)
    for k in PARAMS:
        getattr(g, k).requires_grad_(True)
    T.requires_grad_(True)
    C = 4
    gen = torch.Generator().manual_seed(4)
    f = torch.randn(g.xyz.shape[0], C, generator=gen).to(DEV).requires_grad_(True)
    bg = torch.full((3,), 0.5, device=DEV)
    w = torch.randn(sc.H, sc.W, C, generator=gen).to(DEV) / (sc.W * sc.H)
    fused.keep_last_slab(True)
    try:
        image, fmap, alpha, mask, uv = fused.rasterize_features(g, f, T, cam, sc.near, sc.far, sc.pad, sc.mh, True, bg)
        (fmap * w).sum().backward()
        slab = fused.last_slab()
    finally:
        fused.keep_last_slab(False)
    assert slab is not None and not slab[:, :3].any() and bool(slab[:, 3:].any())
    vis = torch.nonzero(~mask.cpu()).flatten()
    c = lambda x: x.detach().cpu()
    ref, B, E = pose_reference(c(g.xyz)[vis], c(g.quaternion)[vis], c(g.scale)[vis], c(T), c(cam.K), c(slab))
    assert T.grad is not None and tuple(T.grad.shape) == (4, 4) and bool(torch.isfinite(T.grad).all())
    assert not T.grad[3].any() and bool(T.grad[:3].any())
    r = pose_r(T.grad, ref, B, E)
    report("features_pose[feature loss]", r=r)
    assert r <= R_MAX, r
    assert bool(f.grad.any())


# ---- 6. the guards ----------------------------------------------------------------------------------------------------
def test_guards_raise_and_leave_the_next_frame_alone():
    case = frame_case(0.0)
    g, cam, T, bg = frame_inputs(0.0, grads=False)
    f = frame_features(False)
    N = FRAME["N"]
    args = (T, cam, DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"], DEFAULTS["mh_dist"])
    sh = torch.zeros(N, 3, 3, device=DEV)
    g_sh = type(g)(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, sh)
    cpu = lambda x: None if x is None else x.cpu()
    g_cpu = type(g)(cpu(g.xyz), cpu(g.rgb), cpu(g.opacity), cpu(g.scale), cpu(g.quaternion), None)
    g_f64 = type(g)(g.xyz.double(), g.rgb.double(), g.opacity.double(), g.scale.double(), g.quaternion.double(), None)
    rf = fused.rasterize_features
    bad = [
        ("tile_rows", lambda: rf(g, f, *args, True, bg, tile_rows=(0, 2))),
        ("return_aux", lambda: rf(g, f, *args, True, bg, return_aux=True)),
        ("slab_sync", lambda: rf(g, f, *args, True, bg, slab_sync=lambda flat: None)),
        ("grad_sync", lambda: rf(g, f, *args, True, bg, grad_sync=lambda t: None)),
        ("frame_hook", lambda: rf(g, f, *args, True, bg, frame_hook=lambda d: None)),
        ("adam_plan", lambda: rf(g, f, *args, True, bg, adam_plan=object())),
        ("per-pixel SH", lambda: rf(g_sh, f, *args, False, bg)),
        ("CPU", lambda: rf(g_cpu, f.cpu(), cpu(T), type(cam)(cam.width, cam.height, cpu(cam.K)), *args[2:], True, cpu(bg))),
        ("float32", lambda: rf(g_f64, f, T.double(), type(cam)(cam.width, cam.height, cam.K.double()), *args[2:], True,
                               bg.double())),
        # the features themselves
        ("one row per Gaussian", lambda: rf(g, f[:-1], *args, True, bg)),
        ("one row per Gaussian", lambda: rf(g, f[:, 0], *args, True, bg)),
        ("1 to 32 columns", lambda: rf(g, f[:, :0], *args, True, bg)),
        ("1 to 32 columns", lambda: rf(g, torch.zeros(N, 33, device=DEV), *args, True, bg)),
        ("features must be float32", lambda: rf(g, f.double(), *args, True, bg)),
        ("features must be float32", lambda: rf(g, f.cpu(), *args, True, bg)),
    ]
    for words, call in bad:
        with pytest.raises(RuntimeError, match=words):
            call()
        image, fmap, alpha, mask, uv = rf(g, f, *args, True, bg)
        assert torch.equal(image.cpu(), case.image) and torch.equal(uv.cpu(), case.uv), words
        m = forward_measures(dict(feature_map=fmap.cpu(), alpha=alpha.cpu()), case.orc, case.ref, ~case.ref.fragile)
        assert m["r_feature_map"] <= R_MAX and m["r_alpha"] <= R_MAX, (words, m)
    # SH with the precompute mode is supported
    image, fmap, alpha, mask, uv = rf(g_sh, f, *args, True, bg)
    assert bool(torch.isfinite(image).all()) and bool(torch.isfinite(fmap).all())
