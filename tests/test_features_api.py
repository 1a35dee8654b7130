"""The feature-map entry points exist where their callers look for them (no GPU needed): include/gsplat_hip.h declares
gs_render_features / gs_render_features_backward, the built library exports them at ABI 12 with the header's
prototypes, and fused.rasterize_features refuses CPU tensors by name."""
import ctypes
import os
import re

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_render_features", "gs_render_features_backward")


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    lib = _hip.lib()
    P, I = ctypes.c_void_p, ctypes.c_int
    want = {"gs_render_features": [P, P, I, P, P, P, I, I, I, I, P, P, P, P],
            "gs_render_features_backward": [P, P, I, P, P, P, P, P, P, I, I, I, I, P, P, P]}
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(raw, n), n
        assert n in _hip.EXPORTS
        fn = getattr(lib, n)
        assert fn.restype is I and list(fn.argtypes) == want[n], n   # typed from the header, no hand wrapper
    assert lib.gs_abi_version() >= 12


def test_rasterize_features_refuses_cpu_tensors():
    g, cam, T = make_scene(50, 32, 32, 0, seed=1, device="cpu")
    feat = torch.zeros(50, 4)
    with pytest.raises(RuntimeError, match="rasterize_features needs float32 tensors on the GPU"):
        fused.rasterize_features(g, feat, T, cam, use_sh_precompute=True, background_rgb=torch.zeros(3), **DEFAULTS)
