"""The closed form of camera_T_world's gradient (tests/pose_terms.py, what gs_pose_backward computes) against torch
autograd of the float64 per-Gaussian reference with the pose as the leaf.  CPU only."""
import pytest
import torch

from .pose_terms import pose_terms
from .ref64 import general_camera_scene, leaves64, per_gaussian_fp64, random_slab


@pytest.mark.parametrize("kind", ["landscape", "odd", "one_tile_wide"])
@pytest.mark.parametrize("deg", [0, 1, 3])
def test_closed_form_equals_autograd_with_the_pose_as_leaf(kind, deg):
    sc = general_camera_scene(70 + deg, 2000, deg=deg, kind=kind, stress=True)
    L = leaves64(sc.g, requires_grad=False)
    T = sc.T.double().clone().requires_grad_(True)
    out = per_gaussian_fp64(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], T, sc.cam.K, sc.W,
                            sc.H, sc.near, sc.far, sc.pad)
    rows = torch.nonzero(~out["culled"]).flatten()
    assert 0 < rows.numel() < 2000
    slab = random_slab(rows.numel(), 11 + deg)
    y = torch.cat([out["rgb_render"][rows], out["opacity_act"][rows], out["uv"][rows], out["conic"][rows]], dim=1)
    (ref,) = torch.autograd.grad(y, T, grad_outputs=slab.double())
    assert ref.shape == (4, 4) and not ref[3].any()
    g = sc.g
    terms = pose_terms(g.xyz[rows], g.quaternion[rows], g.scale[rows], sc.T, sc.cam.K, slab, torch.float64)
    assert terms.shape == (rows.numel(), 3, 4)
    B = terms.abs().sum(0)
    dev = ((terms.sum(0) - ref[:3]).abs() / B).max()
    print(f"pose closed form [{kind} deg {deg}]: max |sum - autograd| / B = {float(dev):.3g}")
    assert float(dev) <= 1e-10
