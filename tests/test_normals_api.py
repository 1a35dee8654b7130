"""The normals entry points exist where their callers look for them and refuse what they do not serve, by name, without a
device: include/gsplat_hip.h declares the four gs_* functions, the built library exports them at ABI 21 with the header's
prototypes, fused.rasterize_normals has rasterize_features' refusals (and its own for adam_plan), fused.depth_to_normal
and train_ops.normal_consistency_loss validate their arguments."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused, train_ops
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
WANT = {"gs_gaussian_normals": [P, P, P, P, P, I, P, P],
        "gs_gaussian_normals_backward": [P, P, P, P, P, P, I, I, P, P],
        "gs_depth_normal": [P, P, P, I, I, F, I, P, P],
        "gs_depth_normal_backward": [P, P, P, P, I, I, F, I, P, P, P]}


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert "Normals (ABI 21; no reference counterpart)" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    lib = _hip.lib()
    for n, want in WANT.items():
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(raw, n), n
        assert n in _hip.EXPORTS
        fn = getattr(lib, n)
        assert fn.restype is I and list(fn.argtypes) == want, n   # typed from the header, no hand wrapper
    assert lib.gs_abi_version() >= 21


def cpu_frame():
    g, cam, T = make_scene(50, 32, 32, 0, seed=1, device="cpu")
    return g, cam, T, torch.zeros(3)


def test_rasterize_normals_refuses_by_name():
    g, cam, T, bg = cpu_frame()
    call = lambda **kw: fused.rasterize_normals(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS, **kw)
    with pytest.raises(RuntimeError, match="rasterize_normals needs float32 tensors on the GPU"):
        call()
    for kw in (dict(tile_rows=(0, 1)), dict(return_aux=True), dict(grad_sync=lambda t: None),
               dict(slab_sync=lambda t: None), dict(frame_hook=lambda d: None)):
        with pytest.raises(RuntimeError, match="rasterize_normals serves whole single-GPU frames"):
            call(**kw)
    with pytest.raises(RuntimeError, match=r"rasterize_normals does not take the fused optimizer step \(adam_plan\).*"
                                           "quaternion"):
        call(adam_plan=object())
    sh = torch.zeros(50, 3, 3)
    g_sh = type(g)(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, sh)
    with pytest.raises(RuntimeError, match="rasterize_normals needs the SH-precompute colour mode"):
        fused.rasterize_normals(g_sh, T, cam, use_sh_precompute=False, background_rgb=bg, **DEFAULTS)
    with pytest.raises(RuntimeError, match="camera_model"):
        call(camera_model="orthographic")


def test_depth_to_normal_validates():
    cam = SimpleNamespace(K=torch.eye(3))
    d = torch.ones(8, 8)
    with pytest.raises(RuntimeError, match="camera_model"):
        fused.depth_to_normal(d, d, cam, camera_model="orthographic")
    with pytest.raises(RuntimeError, match="depth_to_normal: depth must be float32"):
        fused.depth_to_normal(d, d, cam)
    with pytest.raises(RuntimeError, match="depth_to_normal: depth must be float32"):
        fused.depth_to_normal(d.double(), d, cam)
    with pytest.raises(RuntimeError, match="normal_consistency_loss: normal_map must be"):
        train_ops.normal_consistency_loss(torch.ones(8, 8), d, d, cam)
    with pytest.raises(RuntimeError, match="camera_model"):
        train_ops.normal_consistency_loss(torch.ones(8, 8, 3), d, d, cam, camera_model="orthographic")
