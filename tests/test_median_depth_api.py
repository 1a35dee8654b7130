"""The median-depth entry points exist where their callers look for them (no GPU needed): include/gsplat_hip.h declares
gs_render_median_depth / gs_median_depth_backward with the agreed prototypes, the built library exports them at ABI 22,
_hip types them from the header, fused.rasterize_median_depth refuses by name what it does not serve, and
train_ops.normal_consistency_loss validates as it did before it gained depth_alpha."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from gaussian_splatting_amd import _hip, fused, train_ops
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES = {
    "gs_render_median_depth":
        "const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges, const int32_t* sorted_gaussians, "
        "const int32_t* num_splats_per_pixel, int W, int H, int tile_row0, int tile_row1, void* median_depth, "
        "int32_t* median_index, void* depth, void* alpha, void* transmittance, void* stream",
    "gs_median_depth_backward":
        "const int32_t* median_index, const void* grad_median_depth, int W, int H, int tile_row0, int tile_row1, "
        "void* grad_z, void* stream",
}


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    lib = _hip.lib()
    P, I = ctypes.c_void_p, ctypes.c_int
    want = {"gs_render_median_depth": [P] * 5 + [I] * 4 + [P] * 6,
            "gs_median_depth_backward": [P] * 2 + [I] * 4 + [P] * 2}
    for n, args in PROTOTYPES.items():
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % n, src)
        assert found, n
        assert " ".join(found.group(1).split()) == args, n
        assert hasattr(raw, n), n
        assert n in _hip.EXPORTS
        fn = getattr(lib, n)
        assert fn.restype is I and list(fn.argtypes) == want[n], n   # typed from the header, no hand wrapper
    assert lib.gs_abi_version() >= 22


def test_rasterize_median_depth_refuses_by_name():
    g, cam, T = make_scene(50, 32, 32, 0, seed=1, device="cpu")
    bg = torch.zeros(3)
    kw = dict(use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
    with pytest.raises(RuntimeError, match="rasterize_median_depth needs float32 tensors on the GPU"):
        fused.rasterize_median_depth(g, T, cam, **kw)
    with pytest.raises(RuntimeError, match="rasterize_median_depth serves whole single-GPU frames: tile_rows"):
        fused.rasterize_median_depth(g, T, cam, tile_rows=(0, 1), **kw)
    with pytest.raises(RuntimeError, match=r"rasterize_median_depth does not take the fused optimizer step \(adam_plan\)"):
        fused.rasterize_median_depth(g, T, cam, adam_plan=object(), **kw)
    g_sh = type(g)(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, torch.zeros(50, 3, 3))
    with pytest.raises(RuntimeError, match="rasterize_median_depth needs the SH-precompute colour mode: per-pixel SH"):
        fused.rasterize_median_depth(g_sh, T, cam, **dict(kw, use_sh_precompute=False))
    assert (list(inspect.signature(fused.rasterize_median_depth).parameters)
            == list(inspect.signature(fused.rasterize_rgbd).parameters))


def test_normal_consistency_loss_validates_as_before():
    cam = make_scene(4, 32, 32, 0, seed=1, device="cpu")[1]
    sig = inspect.signature(train_ops.normal_consistency_loss)
    assert list(sig.parameters) == ["normal_map", "depth", "alpha", "camera", "camera_model", "min_alpha", "depth_alpha"]
    assert sig.parameters["depth_alpha"].default is None
    depth = alpha = torch.ones(32, 32)
    for kw in ({}, {"depth_alpha": torch.ones(32, 32)}):
        with pytest.raises(RuntimeError, match=r"normal_consistency_loss: normal_map must be \[H, W, 3\] over depth's"):
            train_ops.normal_consistency_loss(torch.ones(32, 32), depth, alpha, cam, **kw)
        with pytest.raises(RuntimeError, match=r"normal_consistency_loss: normal_map must be \[H, W, 3\] over depth's"):
            train_ops.normal_consistency_loss(torch.ones(16, 32, 3), depth, alpha, cam, **kw)
        # CPU maps reach depth_to_normal's own refusal, worded as before
        with pytest.raises(RuntimeError, match=r"depth_to_normal: depth must be float32 \[H, W\] on the GPU"):
            train_ops.normal_consistency_loss(torch.ones(32, 32, 3), depth, alpha, cam, **kw)
    with pytest.raises(RuntimeError, match="camera_model must be one of"):
        train_ops.normal_consistency_loss(torch.ones(32, 32, 3), depth, alpha, cam, camera_model="orthographic")
