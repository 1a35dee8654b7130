"""The absgrad entry point exists where its callers look for it (no GPU needed): include/gsplat_hip.h declares
gs_render_tiles_backward_slab_abs with the parameter list of gs_render_tiles_backward_slab_m and grad_uv_abs in front of
the stream, the built library exports it at ABI 18, _hip types it from the header, fused.rasterize has the option,
off by default, and refuses by name what the absgrad frame does not serve."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gs_render_tiles_backward_slab_abs"


def _prototype(src, name):
    found = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert found, name
    return " ".join(found.group(1).split())


def test_header_declares_and_library_exports_the_entry_point():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    plain = _prototype(src, "gs_render_tiles_backward_slab_m")
    assert plain.endswith("const uint64_t* touch_masks, void* stream")
    assert _prototype(src, NAME) == plain[:-len("void* stream")] + "void* grad_uv_abs, void* stream"
    raw = ctypes.CDLL(_hip.LIB_PATH)
    lib = _hip.lib()
    assert hasattr(raw, NAME) and NAME in _hip.EXPORTS
    fn, plain_fn = getattr(lib, NAME), lib.gs_render_tiles_backward_slab_m
    assert fn.restype is ctypes.c_int   # typed from the header, no hand wrapper
    assert list(fn.argtypes) == list(plain_fn.argtypes)[:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.gs_abi_version() >= 18


def test_rasterize_has_the_option_off_by_default():
    assert inspect.signature(fused.rasterize).parameters["absgrad"].default is False
    assert inspect.signature(fused.render_backward).parameters["uv_absgrad"].default is None


def test_rasterize_absgrad_refuses_by_name():
    g, cam, T = make_scene(50, 32, 32, 0, seed=1, device="cpu")
    bg = torch.zeros(3)
    kw = dict(use_sh_precompute=True, background_rgb=bg, absgrad=True, **DEFAULTS)
    who = r"rasterize\(absgrad=True\)"
    with pytest.raises(RuntimeError, match=who + " needs float32 tensors on the GPU"):
        fused.rasterize(g, T, cam, **kw)
    with pytest.raises(RuntimeError, match=who + " serves whole single-GPU frames: tile_rows"):
        fused.rasterize(g, T, cam, tile_rows=(0, 1), **kw)
    with pytest.raises(RuntimeError, match=who + " serves whole single-GPU frames"):
        fused.rasterize(g, T, cam, frame_hook=lambda d: None, **kw)
    with pytest.raises(RuntimeError, match=who + r" does not take the fused optimizer step \(adam_plan\)"):
        fused.rasterize(g, T, cam, adam_plan=object(), **kw)
    g_sh = type(g)(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, torch.zeros(50, 3, 3))
    with pytest.raises(RuntimeError, match=who + " needs the SH-precompute colour mode: per-pixel SH"):
        fused.rasterize(g_sh, T, cam, **dict(kw, use_sh_precompute=False))
    with pytest.raises(RuntimeError, match=who + " needs float32 tensors on the GPU"):
        g64 = type(g)(*(t.double() if t is not None else None for t in (g.xyz, g.rgb, g.opacity, g.scale, g.quaternion,
                                                                           g.sh)))
        fused.rasterize(g64, T.double(), cam, **kw)
