"""The contribution statistics without a GPU: tests/contributions_ref.py against the existing float64 reference
(tests/render_ref64.py) on every scene of render_scenes(), the properties of the scenes that the GPU tests
(tests/test_gpu_contributions.py) rely on, and the entry points where their callers look for them.

The two references share no code beyond the tile's pixel grid and the constants: num_splats_per_pixel must be equal,
the sum of pixel_count must be render_fp64's count of contributors, and the sum over the Gaussians of weight_sum must be
the sum over the pixels of the existing reference's accumulated opacity (its image with 1 / Y0 as the colour, the
z-as-colour trick of tests/depth_alpha_ref.py) to 1e-12 relative.  No scene has a fragile pixel."""
import ctypes
import os
import re

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

from . import contributions_ref as C
from . import depth_alpha_ref as D
from . import render_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = list(R.render_scenes())


@pytest.mark.parametrize("name", SCENES)
def test_reference_agrees_with_render_ref64(name):
    sc = D.depth_scene(name)
    old = D.reference(name)
    new = C.reference(name)
    assert torch.equal(new.nsp, old.nsp)
    assert int(new.pixel_count.sum()) == int(old.contrib.sum())
    total, want = float(new.weight_sum.sum()), float(old.alpha.sum())
    assert abs(total - want) <= 1e-12 * abs(want), (total, want)
    assert int(new.fragile.sum()) == 0 and torch.equal(new.fragile, old.fragile)
    # the statistics are consistent among themselves
    touched = new.pixel_count > 0
    assert bool((new.weight_max[touched] >= R.FP32.alpha_min * (1 - R.SAT)).all()) and not new.weight_max[~touched].any()
    assert bool((new.weight_sum >= new.weight_max).all())
    assert bool((new.weight_sum <= new.weight_max * new.pixel_count + 1e-300).all())
    assert new.weight_sum.shape[0] == sc.V


def test_scenes_exercise_what_the_kernel_can_get_wrong():
    """a later edit of the scenes must not hollow the GPU tests"""
    scenes = R.render_scenes()
    ref = C.reference("opaque_stack")          # Gaussians listed but never walked
    assert int(ref.nsp.max()) == 12 and scenes["opaque_stack"].V == 70
    assert int((ref.pixel_count == 0).sum()) >= 70 - 12
    ref = C.reference("faint_300")             # walked visits whose alpha stays below 1 / 255
    assert ref.skipped > 1000 and int(ref.pixel_count.sum()) > 1000
    ref = C.reference("long_1100")             # several chunks of either size, and more than the sorted prefix
    assert R.max_list(scenes["long_1100"]) > _hip.GS_SORT_PREFIX and int(ref.nsp.max()) > _hip.GS_SORT_PREFIX
    for name in ("partial_48x40", "partial_33x17", "strip_70x13", "partial_48x40_black"):
        ref = C.reference(name)                # cross-tile atomics: Gaussians that several tiles list
        shared = int((ref.tiles_of > 1).sum())
        assert 13 <= shared <= 36, (name, shared)
        touched_in_several = int(((ref.tiles_of > 1) & (ref.pixel_count > 0)).sum())
        assert touched_in_several >= 5, (name, touched_in_several)
        assert scenes[name].ranges.numel() - 1 > 1


# ---- the entry points, without a GPU ----------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    lib = _hip.lib()
    P, I = ctypes.c_void_p, ctypes.c_int
    n = "gs_render_contributions"
    assert re.search(r"\bint\s+%s\s*\(" % n, src)
    assert hasattr(raw, n) and n in _hip.EXPORTS
    fn = getattr(lib, n)
    assert fn.restype is I and list(fn.argtypes) == [P, P, P, P, P, I, I, I, I, P, P, P, P]
    assert lib.gs_abi_version() >= 15


def _cpu_frame(n=50):
    g, cam, T = make_scene(n, 32, 32, 0, seed=1, device="cpu")
    return g, cam, T, (g, T, cam, DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"],
                       DEFAULTS["mh_dist"])


def test_rasterize_contributions_refuses_what_it_does_not_serve():
    """RuntimeError naming the reason, before anything is enqueued (there is no GPU here to enqueue on)"""
    g, cam, T, args = _cpu_frame()
    bg = torch.zeros(3)
    with pytest.raises(RuntimeError, match="rasterize_contributions needs float32 tensors on the GPU"):
        fused.rasterize_contributions(*args, True, bg)
    g64 = type(g)(g.xyz.double(), g.rgb.double(), g.opacity.double(), g.scale.double(), g.quaternion.double(), None)
    with pytest.raises(RuntimeError, match="rasterize_contributions needs float32"):
        fused.rasterize_contributions(g64, T.double(), type(cam)(cam.width, cam.height, cam.K.double()), *args[3:], True,
                                      bg.double())
    g_sh = type(g)(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, torch.zeros(50, 3, 3))
    with pytest.raises(RuntimeError, match="rasterize_contributions needs the SH-precompute colour mode"):
        fused.rasterize_contributions(g_sh, *args[1:], False, bg)
    with pytest.raises(RuntimeError, match="rasterize_contributions serves whole single-GPU frames: tile_rows"):
        fused.rasterize_contributions(*args, True, bg, tile_rows=(0, 1))


def test_contribution_stats_record():
    st = fused.ContributionStats.zeros(7, "cpu")
    assert st.frames == 0 and st.n == 7
    assert st.weight_sum.dtype == torch.float32 and st.weight_max.dtype == torch.float32
    assert st.pixel_count.dtype == torch.int32
    assert tuple(st.weight_sum.shape) == tuple(st.weight_max.shape) == tuple(st.pixel_count.shape) == (7,)
    st.pixel_count[2] = 3
    assert st.touched.tolist() == [False, False, True, False, False, False, False]
    # accumulation refuses a changed N: the record of 7 Gaussians cannot take a frame of 50
    g, cam, T, args = _cpu_frame()
    with pytest.raises(RuntimeError, match="change of N"):
        fused.rasterize_contributions(*args, True, torch.zeros(3), stats=st)
    with pytest.raises(RuntimeError, match="must be a ContributionStats"):
        fused.rasterize_contributions(*args, True, torch.zeros(3), stats=(st.weight_sum, st.weight_max, st.pixel_count))
