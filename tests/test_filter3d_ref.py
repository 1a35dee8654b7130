"""The 3D smoothing filter without a GPU: tests/filter3d_ref.py against float64 autograd and tests/ref64.py, fused's torch
helpers (filter3d_from_rate, bake_filter3d), the shares of rows the GPU tests leave out, and the places the feature is
looked for: the header, the loader, the ABI version, the keyword and its refusals."""
import inspect
import re

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.splat_py.structs import Camera, Gaussians
from gaussian_splatting_amd.synthetic import DEFAULTS

from . import filter3d_ref as F
from .fisheye_ref import leaves
from .ref64 import per_gaussian_fp64

LEFT_OUT_MAX = 0.005   # tests/test_gpu_antialias.py


def rows_2000():
    """2 000 rows with phi spread over eight decades around the row's scales (and some exact zeros)"""
    gen = torch.Generator().manual_seed(5)
    n = 2000
    log_s = (-4.0 + 3.0 * torch.randn(n, 3, generator=gen, dtype=torch.float64))
    logit = 3.0 * torch.randn(n, generator=gen, dtype=torch.float64)
    s2max = (torch.exp(log_s) ** 2).max(dim=1).values
    phi = s2max * 10.0 ** (-6.0 + 8.0 * torch.rand(n, generator=gen, dtype=torch.float64))
    phi[::50] = 0.0
    return log_s, logit, phi


def test_closed_forms_against_autograd():
    log_s, logit, phi = rows_2000()
    log_s.requires_grad_(True)
    logit.requires_grad_(True)
    opa3 = torch.sigmoid(logit) * F.comp3_of(log_s, phi)
    g = torch.randn(opa3.shape[0], generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    a_s, a_o = torch.autograd.grad(opa3, [log_s, logit], grad_outputs=g)
    go, gs = F.closed_form_terms(log_s.detach(), logit.detach(), phi, g)
    row = torch.cat([a_s, a_o[:, None]], dim=1).abs().max(dim=1).values
    err = torch.cat([(gs - a_s).abs(), (go - a_o).abs()[:, None]], dim=1).max(dim=1).values
    worst = float((err / row.clamp(min=1e-300)).max())
    print(f"filter3d closed forms against autograd: worst relative error {worst:.3g}")
    assert worst <= 1e-9
    # the invariant opa3 sqrt(prod (s^2 + phi)) = y prod s
    s2 = torch.exp(log_s.detach()) ** 2
    lhs = opa3.detach() * torch.sqrt((s2 + phi[:, None]).prod(dim=1))
    rhs = torch.sigmoid(logit.detach()) * torch.sqrt(s2.prod(dim=1))
    assert float(((lhs - rhs).abs() / rhs).max()) <= 1e-12
    # fp32: no cancellation in the factor
    o32 = torch.sigmoid(logit.detach().float()) * F.comp3_of(log_s.detach().float(), phi.float())
    o64 = torch.sigmoid(logit.detach().float().double()) * F.comp3_of(log_s.detach().float().double(), phi.float().double())
    assert float(((o32.double() - o64).abs() / o64).max()) < 2e-6


@pytest.mark.parametrize("kind", [k for k, _ in F.SCENES])
def test_phi_zero_is_ref64_exactly(kind):
    sc = F.scene(kind)
    L = leaves(sc.g, torch.float64, requires_grad=False)
    want = per_gaussian_fp64(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], sc.T, sc.cam.K, sc.W,
                             sc.H, sc.near, sc.far, sc.pad)
    got = F.stage(sc, torch.zeros_like(sc.phi), torch.float64)
    none = F.stage(sc, None, torch.float64)
    for k in want:
        assert torch.equal(got[k], want[k]) and torch.equal(none[k], want[k]), k
    assert torch.equal(got["opa"], want["opacity_act"])
    # the scene's filter has the three regimes the issue names
    s2max = (torch.exp(sc.g.scale.double()) ** 2).max(dim=1).values
    ratio = sc.phi.double() / s2max.clamp(min=1e-300)
    n = sc.phi.shape[0]
    assert 0.015 * n < int((sc.phi == 0).sum()) < 0.05 * n and 0.015 * n < int((ratio > 1e5).sum()) < 0.05 * n


def test_bake_against_the_filtered_stage_and_by_hand():
    # by hand: s = (1, 2, 0.5), phi = 3, logit 0:  s^2 + phi = (4, 7, 3.25), comp3 = sqrt(1/4 * 4/7 * 0.25/3.25)
    g = Gaussians(torch.zeros(1, 3, dtype=torch.float64), torch.ones(1, 3, dtype=torch.float64),
                  torch.zeros(1, 1, dtype=torch.float64),
                  torch.log(torch.tensor([[1.0, 2.0, 0.5]], dtype=torch.float64)),
                  torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64))
    b = fused.bake_filter3d(g, torch.tensor([3.0], dtype=torch.float64))
    comp3 = (0.25 * (4.0 / 7.0) * (0.25 / 3.25)) ** 0.5
    assert torch.allclose(torch.exp(b.scale) ** 2, torch.tensor([[4.0, 7.0, 3.25]], dtype=torch.float64), rtol=1e-14)
    assert abs(float(torch.sigmoid(b.opacity)) - 0.5 * comp3) < 1e-15
    assert b.xyz is g.xyz and b.quaternion is g.quaternion and b.rgb is g.rgb
    # against the filtered stage: the classic stage of the baked Gaussians is the filtered stage of the originals
    sc = F.scene("odd")
    L = leaves(sc.g, torch.float64, requires_grad=False)
    g64 = Gaussians(L["xyz"], L["rgb"], L["opacity"], L["scale"], L["quaternion"], L["sh"])
    baked = fused.bake_filter3d(g64, sc.phi.double())
    want = F.stage(sc, sc.phi, torch.float64)
    got = per_gaussian_fp64(baked.xyz, baked.quaternion, baked.scale, baked.opacity, baked.rgb, baked.sh, sc.T, sc.cam.K,
                            sc.W, sc.H, sc.near, sc.far, sc.pad)
    ok = want["comp3"] > 1e-150     # (below, logit(opa3) leaves float64's range)
    assert float(ok.double().mean()) > 0.99
    for a, b_ in ((got["conic"], want["conic"]), (got["opacity_act"], want["opa"])):
        rel = (a[ok] - b_[ok]).abs() / b_[ok].abs().max(dim=1, keepdim=True).values.clamp(min=1e-300)
        assert float(rel.max()) < 1e-9
    # differentiable
    s = g64.scale.clone().requires_grad_(True)
    out = fused.bake_filter3d(Gaussians(g64.xyz, g64.rgb, g64.opacity, s, g64.quaternion, g64.sh), sc.phi.double())
    out.scale[ok].sum().backward()
    assert bool(torch.isfinite(s.grad).all()) and bool(s.grad.any())


def test_from_rate():
    rate = torch.tensor([0.0, 2.0, 4.0, 0.0, 0.5])
    got = fused.filter3d_from_rate(rate, variance=0.2)
    assert torch.equal(got, F.from_rate(rate, 0.2))
    assert torch.allclose(got, torch.tensor([0.8, 0.05, 0.0125, 0.8, 0.8]))
    assert torch.equal(fused.filter3d_from_rate(torch.zeros(7)), torch.zeros(7))
    assert fused.filter3d_from_rate(torch.zeros(0)).shape == (0,)
    sig = inspect.signature(fused.filter3d_from_rate)
    assert sig.parameters["variance"].default == 0.2
    sig = inspect.signature(fused.filter3d_rate)
    assert (sig.parameters["near_thresh"].default, sig.parameters["pad_fraction"].default) == (0.2, 0.15)


# ---- the shares the GPU tests leave out, for the reference alone ----------------------------------------------------------
@pytest.mark.parametrize("fisheye", [False, True])
@pytest.mark.parametrize("C", F.CAMERA_COUNTS)
def test_rate_left_out_share(C, fisheye):
    """outside the rows within EDGE_PX of a padded edge or NEAR_REL of near in some camera, the fp32 and float64
    restatements see the same cameras; those rows are few, and some rows are never seen (the fallback of from_rate)"""
    sc, cams = F.scene("landscape"), F.camera_set("landscape", C)
    r64, seen64, fragile = F.rate_of(sc.g.xyz, cams.Ts, cams.Ks, cams.sizes, fisheye=fisheye, detail=True)
    r32, seen32, _ = F.rate_of(sc.g.xyz, cams.Ts, cams.Ks, cams.sizes, dtype=torch.float32, fisheye=fisheye, detail=True)
    n = r64.shape[0]
    differs = (seen64 != seen32).any(dim=0)
    never = int((r64 == 0).sum())
    print(f"filter3d rate C = {C} fisheye = {fisheye}: {int(fragile.sum())} of {n} rows left out, "
          f"{int(differs.sum())} decisions differ, {never} rows never seen")
    assert int(fragile.sum()) <= LEFT_OUT_MAX * n
    assert not bool((differs & ~fragile).any())
    if C < 67:
        assert 0 < never < n    # the fallback of from_rate is exercised
    rel = ((r32.double() - r64).abs() / r64.clamp(min=1e-300))[~fragile & (r64 > 0)]
    assert float(rel.max()) < 1e-4
    phi = F.from_rate(r64)
    assert bool((phi[r64 == 0] == phi[r64 > 0].max()).all())


@pytest.mark.parametrize("kind", [k for k, _ in F.SCENES])
def test_antialiased_left_out_share(kind):
    """under antialiased, the rows whose det_0 > 0 decision differs between the fp32 and the float64 restatement (7e)"""
    sc = F.scene(kind)
    for mode in ("filter+aa", "filter+aa+fisheye"):
        o64, o32 = F.stage(sc, sc.phi, torch.float64, mode), F.stage(sc, sc.phi, torch.float32, mode)
        vis = ~o64["culled"]
        flips = ((o64["det_0"] > 0) != (o32["det_0"] > 0)) & vis
        print(f"filter3d {kind} {mode}: det_0 flips on {int(flips.sum())} of {int(vis.sum())} visible rows")
        assert int(flips.sum()) <= LEFT_OUT_MAX * int(vis.sum())


# ---- header, loader, keyword, refusals ---------------------------------------------------------------------------------
ENTRY_POINTS = (fused.rasterize, fused.rasterize_rgbd, fused.rasterize_distortion, fused.rasterize_features,
                fused.rasterize_contributions, fused.preprocess_forward, fused.preprocess_backward, fused.pose_backward)


def test_header_loader_and_abi():
    lib = _hip.lib()
    assert lib.gs_abi_version() >= 20
    src = open(_hip.HEADER_PATH).read()
    flat = re.sub(r"\s+", " ", src)
    for name, tail in (("gs_preprocess_forward_filtered", "int sample_stride, const void* filter3d, int raster_mode, void* stream"),
                       ("gs_preprocess_backward_filtered", "void* grad_sh, const void* filter3d, int raster_mode, void* stream"),
                       ("gs_pose_backward_filtered", "void* grad_camera_T_world, const void* filter3d, int raster_mode, void* stream"),
                       ("gs_filter3d_rate", "int raster_mode, void* rate, void* stream")):
        m = re.search(r"int %s\(([^)]*)\);" % name, flat)
        assert m and m.group(1).endswith(tail), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(m.group(1).split(",")), name
    # the _mode prototypes are the ones of ABI 19
    for name, tail in (("gs_preprocess_forward_mode", "int sample_stride, int raster_mode, void* stream"),
                       ("gs_preprocess_backward_mode", "void* grad_sh, int raster_mode, void* stream"),
                       ("gs_pose_backward_mode", "void* grad_camera_T_world, int raster_mode, void* stream")):
        m = re.search(r"int %s\(([^)]*)\);" % name, flat)
        f = re.search(r"int %s\(([^)]*)\);" % name.replace("_mode", "_filtered"), flat)
        assert m and m.group(1).endswith(tail), name
        assert f.group(1).replace(" const void* filter3d,", "") == m.group(1), name
    assert "rho3 > 0 ? sqrt(rho3) : 0" in src and "3D smoothing filter" in src
    assert (_hip.GS_RASTER_CLASSIC, _hip.GS_RASTER_ANTIALIASED, _hip.GS_RASTER_FISHEYE) == (0, 1, 2)
    assert len(inspect.signature(fused._raster_mode).parameters) == 2


def test_keyword_is_on_the_entry_points_and_off_by_default():
    for fn in ENTRY_POINTS:
        par = inspect.signature(fn).parameters
        assert "filter3d" in par and par["filter3d"].default is None, fn.__name__
    assert inspect.signature(fused._frame_record).parameters["filter3d"].default is None
    for name in ("filter3d_rate", "filter3d_from_rate", "bake_filter3d"):
        assert callable(getattr(fused, name))


def test_refusals_on_cpu_tensors():
    n = 10
    g = Gaussians(torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n, 1), torch.zeros(n, 3), torch.ones(n, 4))
    cam, T, bg = Camera(32, 32, torch.eye(3)), torch.eye(4), torch.zeros(3)
    phi = torch.zeros(n)
    for fn in (fused.rasterize, fused.rasterize_rgbd, fused.rasterize_distortion, fused.rasterize_contributions):
        with pytest.raises(RuntimeError, match="float32 tensors on the GPU"):
            fn(g, T, cam, use_sh_precompute=True, background_rgb=bg, filter3d=phi, **DEFAULTS)
    with pytest.raises(RuntimeError, match="float32 tensors on the GPU"):
        fused.rasterize_features(g, torch.zeros(n, 2), T, cam, use_sh_precompute=True, background_rgb=bg, filter3d=phi,
                                 **DEFAULTS)
    for kw, what in ((dict(tile_rows=(0, 1)), "tile_rows"), (dict(return_aux=True), "return_aux"),
                     (dict(grad_sync=lambda t: t), "grad_sync"), (dict(slab_sync=lambda t: None), "slab_sync"),
                     (dict(frame_hook=lambda d: None), "frame_hook"), (dict(adam_plan=object()), "adam_plan")):
        with pytest.raises(RuntimeError, match=r"filter3d.*" + what):
            fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, filter3d=phi, **kw, **DEFAULTS)
    gsh = Gaussians(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, torch.zeros(n, 3, 3))
    with pytest.raises(RuntimeError, match="filter3d.*per-pixel SH"):
        fused.rasterize(gsh, T, cam, use_sh_precompute=False, background_rgb=bg, filter3d=phi, **DEFAULTS)
    with pytest.raises(RuntimeError, match="filter3d.*tile_rows"):
        fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, None, T, cam.K, 32, 32, 0.3, 500.0, 100,
                                 3.0, (0, 1), 0, filter3d=phi)
    with pytest.raises(RuntimeError, match="xyz must be float32"):
        fused.filter3d_rate(g.xyz, T[None], cam.K[None], (32, 32))
    # the C entry refuses a band with a filter by name, before anything is launched
    lib = _hip.lib()
    one = 1 << 12   # (any non-NULL address: the refusal comes first)
    args = [one] * 6 + [1, one, one, n, 32, 32, 0.3, 500.0, 100.0, 3.0, 0, 1] + [one] * 12 + [None, None, None, 0]
    assert lib.gs_preprocess_forward_filtered(*args, one, 0, None) == _hip.GS_EINVAL
    assert b"filter3d" in lib.gs_last_error()
    assert lib.gs_preprocess_forward_filtered(*args, one, 4, None) == _hip.GS_EINVAL
    assert b"raster_mode" in lib.gs_last_error()
    assert lib.gs_filter3d_rate(one, one, one, None, 1, n, 0.2, 0.15, 0, one, None) == _hip.GS_EINVAL
    assert lib.gs_filter3d_rate(one, one, one, None, 1, n, 0.2, 0.15, 1, one, None) == _hip.GS_EINVAL
    assert b"raster_mode" in lib.gs_last_error()
    assert lib.gs_filter3d_rate(None, None, None, None, 0, n, 0.2, 0.15, 0, None, None) == _hip.GS_OK
    assert lib.gs_filter3d_rate(None, None, None, None, 3, 0, 0.2, 0.15, 2, None, None) == _hip.GS_OK
