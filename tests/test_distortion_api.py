"""The depth-distortion entry points exist where their callers look for them (no GPU needed): include/gsplat_hip.h
declares gs_render_distortion / gs_render_distortion_backward with the agreed prototypes, the built library exports
them at ABI 16, _hip types them from the header, and fused.rasterize_distortion refuses by name what it does not
serve."""
import ctypes
import os
import re

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES = {
    "gs_render_distortion":
        "const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges, const int32_t* sorted_gaussians, "
        "const int32_t* num_splats_per_pixel, int W, int H, int tile_row0, int tile_row1, void* distortion, "
        "void* depth, void* alpha, void* transmittance, void* stream",
    "gs_render_distortion_backward":
        "const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges, const int32_t* sorted_gaussians, "
        "const int32_t* num_splats_per_pixel, const void* transmittance, const void* depth, const void* alpha, "
        "const void* grad_distortion, const void* grad_depth, const void* grad_alpha, int W, int H, int tile_row0, "
        "int tile_row1, void* grad_slab, void* grad_z, void* stream",
}


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    lib = _hip.lib()
    P, I = ctypes.c_void_p, ctypes.c_int
    want = {"gs_render_distortion": [P] * 5 + [I] * 4 + [P] * 5,
            "gs_render_distortion_backward": [P] * 11 + [I] * 4 + [P] * 3}
    for n, args in PROTOTYPES.items():
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % n, src)
        assert found, n
        assert " ".join(found.group(1).split()) == args, n
        assert hasattr(raw, n), n
        assert n in _hip.EXPORTS
        fn = getattr(lib, n)
        assert fn.restype is I and list(fn.argtypes) == want[n], n   # typed from the header, no hand wrapper
    assert lib.gs_abi_version() >= 16


def test_rasterize_distortion_refuses_by_name():
    g, cam, T = make_scene(50, 32, 32, 0, seed=1, device="cpu")
    bg = torch.zeros(3)
    kw = dict(use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
    with pytest.raises(RuntimeError, match="rasterize_distortion needs float32 tensors on the GPU"):
        fused.rasterize_distortion(g, T, cam, **kw)
    with pytest.raises(RuntimeError, match="rasterize_distortion serves whole single-GPU frames: tile_rows"):
        fused.rasterize_distortion(g, T, cam, tile_rows=(0, 1), **kw)
    with pytest.raises(RuntimeError, match=r"rasterize_distortion does not take the fused optimizer step \(adam_plan\)"):
        fused.rasterize_distortion(g, T, cam, adam_plan=object(), **kw)
    g_sh = type(g)(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, torch.zeros(50, 3, 3))
    with pytest.raises(RuntimeError, match="rasterize_distortion needs the SH-precompute colour mode: per-pixel SH"):
        fused.rasterize_distortion(g_sh, T, cam, **dict(kw, use_sh_precompute=False))
