"""The reference of the depth / alpha maps (gs_render_zalpha, fused.rasterize_rgbd): tests/render_ref64.py itself, fed
the camera-frame z as a colour (test code only).

With one colour coefficient the reference's colour is Y0 * coeff, so coeff = (z / Y0, 1 / Y0, 0), background 0 and
grad_image = (g_depth, g_alpha, 0) make

  image[..., 0] = sum w_k z_k = depth        image[..., 1] = sum w_k = alpha
  grad["g_rgb"][:, 0] / Y0 = dL/dz           grad["g_opacity" | "g_uv" | "g_conic"] = the slab's columns 3..8

and the same for the abs sums.  `grad` is the true derivative, which the depth kernels are held to; `grad_walk` (the
reference walk's gradient, scaled by 1 / (1 - alpha_last) where skipped entries trail the last contributor) is kept to
show that the two can be told apart on these scenes.  The scenes are render_ref64.render_scenes() with a seeded
z = 1 + 9 rand(V) per scene; g_depth and g_alpha are the first two channels of the scene's grad_image.  The reference
gets the coefficients in float64 (its depth is the depth of the fp32 z values), the fp32 oracle the same rounded to
fp32."""
import functools
from types import SimpleNamespace

import torch

from . import render_ref64 as R
from .ref64 import sh_basis
from .test_gpu_render_ref64 import noise_measure   # noqa: F401 (the measure of the gradient checks, re-exported)

Y0 = float(sh_basis(torch.zeros(1, 3, dtype=torch.float64), 1)[0, 0])
KEYS = ("g_z", "g_opacity", "g_uv", "g_conic")


def z_coeff(z):
    """[V, 3] float64 coefficients (z / Y0, 1 / Y0, 0) of fp32 depths z [V]"""
    z = z.detach().double().cpu()
    return torch.stack([z / Y0, torch.full_like(z, 1 / Y0), torch.zeros_like(z)], dim=1)


def as_depth_scene(sc, z, grad_image):
    """scene sc (render_ref64._scene's fields) with z [V] in place of its colour, background 0 and grad_image's third
    channel cleared"""
    d = SimpleNamespace(**vars(sc))
    d.z = z.detach().float().cpu().contiguous()
    d.coeff64 = z_coeff(d.z)
    d.coeff16 = d.coeff64.float().reshape(-1, 3, 1).contiguous()   # what render_ref64.scene_coeff hands the oracle
    d.bg = torch.zeros(3)
    d.grad_image = grad_image.detach().float().cpu().clone()
    d.grad_image[..., 2] = 0
    return d


@functools.lru_cache(maxsize=None)
def depth_scene(name):
    sc = R.render_scenes()[name]
    gen = torch.Generator().manual_seed(5000 + list(R.render_scenes()).index(name))
    z = 1 + 9 * torch.rand(sc.V, generator=gen, dtype=torch.float64)
    return as_depth_scene(sc, z.float(), sc.grad_image)


def fields(out):
    """depth / alpha / the four gradients out of a render result in render_ref64's naming (a dict of tensors: the
    oracle's or a kernel's run_module output, or one of the reference's grad / abs dicts)"""
    res = {}
    if "image" in out:
        res.update(depth=out["image"][..., 0], alpha=out["image"][..., 1])
    if "g_rgb" in out:
        res.update(g_z=out["g_rgb"].reshape(out["g_rgb"].shape[0], 3, -1)[:, 0, 0] / Y0, g_opacity=out["g_opacity"],
                   g_uv=out["g_uv"], g_conic=out["g_conic"])
    return res


def reference_of(sc, grad_image):
    """render_fp64 (FP32 settings) of depth scene sc for grad_image -> the reference's namespace plus depth, alpha
    [H, W] and grad / grad_walk / abs / abs_walk re-keyed to KEYS"""
    ref = R.render_fp64(sc.uv, sc.opacity, sc.coeff64, sc.conic, sc.rays, sc.ranges, sc.sorted_g, sc.bg, sc.W, sc.H,
                        R.FP32, grad_image)
    ref.grad_image = (grad_image.double() * (~ref.fragile)[:, :, None]).contiguous()
    ref.depth, ref.alpha = ref.image[..., 0], ref.image[..., 1]
    for k in ("grad", "grad_walk", "abs", "abs_walk"):
        setattr(ref, k, fields(getattr(ref, k)))
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, unscaled_only=False):
    """the reference of scene `name`; unscaled_only: grad_image is zero on the pixels whose walk gradient is scaled too
    (there the fp32 oracle's gradient is the true derivative).  Computed once; do not modify."""
    sc = depth_scene(name)
    gi = sc.grad_image
    if unscaled_only:
        gi = gi * (reference(name).scale == 1)[:, :, None]
    return reference_of(sc, gi)

