"""The fisheye reference of tests/fisheye_ref.py against itself and against the pinhole reference (no GPU needed), and
the places the fisheye mode is looked for: the header's constant, the loader, the ABI version, fused's keyword and its
refusals."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

from . import fisheye_ref as F
from .ref64 import leaves64, per_gaussian_fp64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX, FY, CX, CY = 500.0, 430.0, 310.0, 250.0


def directions(theta, phi, z=2.0):
    """camera-frame points at angle theta from the axis, azimuth phi, depth z (float64)"""
    r = z * torch.tan(theta)
    return torch.stack([r * torch.cos(phi), r * torch.sin(phi), torch.full_like(r, z)], dim=1)


def test_closed_form_jacobian_is_the_derivative_of_the_projection():
    gen = torch.Generator().manual_seed(1)
    n = 400
    theta = math.radians(88.0) * torch.rand(n, generator=gen, dtype=torch.float64)
    theta[:8] = torch.tensor([0.0, 1e-8, 1e-6, 1e-4, 1e-3, 1e-2, 0.0316, 0.0317], dtype=torch.float64)
    phi = 2 * math.pi * torch.rand(n, generator=gen, dtype=torch.float64)
    c = directions(theta, phi, z=0.5 + 20 * torch.rand(n, generator=gen, dtype=torch.float64)[0]).requires_grad_(True)
    uv = F.project(c, FX, FY, CX, CY)
    auto = torch.stack([torch.autograd.grad(uv[:, k].sum(), c, retain_graph=True)[0] for k in (0, 1)], dim=1)
    J = F.jacobian(c.detach(), FX, FY)
    err = ((J - auto).abs().amax(dim=2) / auto.abs().amax(dim=2)).max()
    assert float(err) < 1e-12, float(err)


def test_optical_axis_limits_and_continuity():
    z = 3.0
    c0 = torch.tensor([[0.0, 0.0, z]], dtype=torch.float64)
    s, a, q, d = F.fisheye_terms(c0, with_d=True)
    assert float(s) == 1 / z and float(q) == 1 / (z * z)
    assert abs(float(a) - (-2 / (3 * z ** 3))) < 1e-16 and abs(float(d) - 8 / (5 * z ** 5)) < 1e-16
    assert torch.equal(F.project(c0, FX, FY, CX, CY), torch.tensor([[CX, CY]], dtype=torch.float64))
    J0 = F.jacobian(c0, FX, FY)[0]
    want = torch.tensor([[FX / z, 0.0, 0.0], [0.0, FY / z, 0.0]], dtype=torch.float64)
    assert float((J0 - want).abs().max()) < 1e-13 and bool((J0[want == 0] == 0).all())
    for e in range(-8, 0):
        theta = torch.tensor([10.0 ** e], dtype=torch.float64)
        c = directions(theta, torch.tensor([0.7], dtype=torch.float64), z)
        s1, a1, q1, d1 = F.fisheye_terms(c, with_d=True)
        tol = 3 * float(theta) ** 2 + 1e-15   # the terms are even in theta
        assert abs(float(s1 / s) - 1) < tol and abs(float(a1 / a) - 1) < tol and abs(float(d1 / d) - 1) < 4 * tol
        J = F.jacobian(c, FX, FY)[0]
        assert float((J - J0).abs().max()) < FX * (2 * float(theta) + 1e-15)
    # both sides of the series threshold agree (float64: closed form and series)
    w = F.SERIES_W
    for k in (0.999, 1.001):
        c = torch.tensor([[z * math.sqrt(w * k), 0.0, z]], dtype=torch.float64)
        _, a2, q2, d2 = F.fisheye_terms(c, with_d=True)
        s2 = math.atan2(float(c[0, 0]), z) / float(c[0, 0])
        assert abs(float(a2) - (z * float(q2) - s2) / float(c[0, 0]) ** 2) < 1e-10 * abs(float(a2))
        assert abs(float(d2) + (2 * z * float(q2) ** 2 + 3 * float(a2)) / float(c[0, 0]) ** 2) < 1e-7 * abs(float(d2))


def test_small_angles_approach_the_pinhole_model_as_theta_squared():
    sc = F.scene("landscape")
    rows = torch.arange(64)
    errs = []
    for theta in (1e-2, 1e-3):
        L = leaves64(sc.g, requires_grad=False)
        gen = torch.Generator().manual_seed(2)
        phi = 2 * math.pi * torch.rand(64, generator=gen, dtype=torch.float64)
        c = directions(torch.full((64,), theta, dtype=torch.float64), phi, 5.0)
        A, t = sc.T.double()[:3, :3], sc.T.double()[:3, 3]
        xyz = (c - t) @ A   # A orthonormal: A^T (c - t)
        args = (xyz, L["quaternion"][rows], L["scale"][rows], L["opacity"][rows], L["rgb"][rows],
                None if L["sh"] is None else L["sh"][rows], sc.T, sc.cam.K, sc.W, sc.H, sc.near, sc.far, sc.pad)
        pin, fish = per_gaussian_fp64(*args), F.per_gaussian_fisheye(*args)
        K = sc.cam.K.double()
        e_uv = ((fish["uv"] - pin["uv"]).abs() / (pin["uv"] - K[:2, 2]).abs().clamp(min=1e-300)).max()
        e_conic = ((fish["conic"] - pin["conic"]).abs().amax(1) / pin["conic"].abs().amax(1)).max()
        errs.append((float(e_uv), float(e_conic)))
        assert float(e_uv) < theta ** 2 and float(e_conic) < 4 * theta ** 2, (theta, errs)
    assert errs[1][0] < errs[0][0] / 50 and errs[1][1] < errs[0][1] / 50, errs


@pytest.mark.parametrize("name", F.SCENES)
def test_left_out_rows_are_few_in_the_reference(name):
    """the rows the GPU tests leave out (tests/fisheye_ref.py: left_out) are under 0.5 % of the visible rows, and the
    float32 evaluation of the reference decides every other row as float64 does"""
    sc = F.scene(name)
    ref, f32 = F.stage(sc, torch.float64), F.stage(sc, torch.float32)
    out = F.left_out(ref, sc)
    V = int((~ref["culled"]).sum())
    assert V > 1000 and int((out & ~ref["culled"]).sum()) < 0.005 * V, (int(out.sum()), V)
    assert torch.equal(f32["culled"][~out], ref["culled"][~out])
    assert bool(torch.isfinite(ref["conic"][~ref["culled"]]).all())
    if name == "wide":
        u = ref["uv"][:, 0] - float(sc.cam.K[0, 2])
        beyond = float((u.abs() > sc.W / 2 + sc.pad).double().mean())
        assert 0.1 < beyond < 0.25, beyond
        axis = sc.rows["optical_axis"]
        assert not ref["xyz_cam"][axis, :2].any() and not ref["culled"][axis].any()


def test_header_constant_loader_and_abi():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert re.search(r"^#define GS_RASTER_FISHEYE 2$", src, flags=re.M)
    assert (_hip.GS_RASTER_CLASSIC, _hip.GS_RASTER_ANTIALIASED, _hip.GS_RASTER_FISHEYE) == (0, 1, 2)
    lib = _hip.lib()
    assert lib.gs_abi_version() >= 19
    raw = ctypes.CDLL(_hip.LIB_PATH)
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, tail in (("gs_preprocess_forward_mode", "int sample_stride, int raster_mode, void* stream"),
                       ("gs_preprocess_backward_mode", "void* grad_sh, int raster_mode, void* stream"),
                       ("gs_pose_backward_mode", "void* grad_camera_T_world, int raster_mode, void* stream")):
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert found and " ".join(found.group(1).split()).endswith(tail), name
        assert hasattr(raw, name) and name in _hip.EXPORTS
        assert list(getattr(lib, name).argtypes)[-2:] == [ctypes.c_int, ctypes.c_void_p]
    assert not [n for n in _hip.EXPORTS if "fisheye" in n]   # no new entry points: the three _mode entries carry the flag


def test_keyword_defaults():
    for fn in (fused.rasterize, fused.rasterize_rgbd, fused.rasterize_distortion, fused.rasterize_features,
               fused.rasterize_contributions, fused.preprocess_forward, fused.preprocess_backward, fused.pose_backward):
        assert inspect.signature(fn).parameters["camera_model"].default == "pinhole", fn.__name__


def test_fisheye_refuses_by_name_and_unknown_models_list_both():
    g, cam, T = make_scene(50, 32, 32, 0, seed=1, device="cpu")
    bg = torch.zeros(3)
    kw = dict(use_sh_precompute=True, background_rgb=bg, camera_model="fisheye", **DEFAULTS)
    who = r'rasterize\(camera_model="fisheye"\)'
    with pytest.raises(RuntimeError, match=who + " needs float32 tensors on the GPU"):
        fused.rasterize(g, T, cam, **kw)
    with pytest.raises(RuntimeError, match=who + " serves whole single-GPU frames: tile_rows"):
        fused.rasterize(g, T, cam, tile_rows=(0, 1), **kw)
    for hook in (dict(frame_hook=lambda d: None), dict(return_aux=True), dict(grad_sync=lambda t: t),
                 dict(slab_sync=lambda t: None)):
        with pytest.raises(RuntimeError, match=who + " serves whole single-GPU frames"):
            fused.rasterize(g, T, cam, **hook, **kw)
    with pytest.raises(RuntimeError, match=who + r" does not take the fused optimizer step \(adam_plan\)"):
        fused.rasterize(g, T, cam, adam_plan=object(), **kw)
    g_sh = type(g)(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, torch.zeros(50, 3, 3))
    with pytest.raises(RuntimeError, match=who + " needs the SH-precompute colour mode: per-pixel SH"):
        fused.rasterize(g_sh, T, cam, **dict(kw, use_sh_precompute=False))
    g64 = type(g)(*(t.double() if t is not None else None for t in (g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, g.sh)))
    with pytest.raises(RuntimeError, match=who + " needs float32 tensors on the GPU"):
        fused.rasterize(g64, T.double(), cam, **kw)
    for fn, name in ((fused.rasterize_rgbd, "rasterize_rgbd"), (fused.rasterize_distortion, "rasterize_distortion"),
                     (fused.rasterize_contributions, "rasterize_contributions")):
        with pytest.raises(RuntimeError, match=name + " needs float32 tensors on the GPU"):
            fn(g, T, cam, **kw)
    with pytest.raises(RuntimeError, match="tile_rows"):
        fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, 32, 32, 0.3, 500.0, 100,
                                 3.0, (0, 1), 0, camera_model="fisheye")
    for fn in (fused.rasterize, fused.rasterize_rgbd, fused.rasterize_distortion, fused.rasterize_contributions):
        with pytest.raises(RuntimeError, match="'pinhole' / 'fisheye'.*'orthographic'"):
            fn(g, T, cam, **dict(kw, camera_model="orthographic"))
    with pytest.raises(RuntimeError, match="'pinhole' / 'fisheye'"):
        fused.rasterize_features(g, torch.zeros(50, 2), T, cam, **dict(kw, camera_model="equisolid"))
