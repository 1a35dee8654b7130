"""The reference of the feature maps (gs_render_features, fused.rasterize_features): tests/render_ref64.py itself, fed
the feature channels as colours three at a time (test code only), as tests/depth_alpha_ref.py feeds it z.

render_fp64 composites three channels per call.  The C + 1 channels [features | 1] (the constant one is alpha) are
zero-padded to a multiple of three and cut into groups of three; with one colour coefficient the reference's colour is
Y0 * coeff, so coeff = channels / Y0, background 0 and grad_image = the matching three channels of [g_F | g_alpha | 0]
make, per group,

  image = the three maps        grad["g_rgb"] / Y0 = dL/d(channel rows)        g_opacity | g_uv | g_conic = its share

and the shares of the groups ADD (so do the abs sums): the derivative is linear in the output gradient and no decision
depends on the channels -- fragile, nsp and scale are the same from group to group.  `grad` is the true derivative,
which the feature kernels are held to; `grad_walk` is kept to show that the two can be told apart.  The scenes are
render_ref64.render_scenes() with seeded features = randn(V, C) and [g_F | g_alpha] = randn(H, W, C + 1) per scene and
channel count.  The reference gets the fp32 feature values in float64, the fp32 oracle (group by group, combined the
same way) the coefficients rounded to fp32."""
import functools
from types import SimpleNamespace

import torch

from . import render_ref64 as R
from .depth_alpha_ref import Y0
from .test_gpu_render_ref64 import noise_measure   # noqa: F401 (the measure of the gradient checks, re-exported)

KEYS = ("g_features", "g_opacity", "g_uv", "g_conic")
SHARED = ("g_opacity", "g_uv", "g_conic")


def n_groups(C):
    return (C + 1 + 2) // 3


def _padded(x, C):
    """[..., C + 1] -> [..., 3 * n_groups(C)] with zeros behind"""
    pad = 3 * n_groups(C) - (C + 1)
    return torch.cat([x, x.new_zeros(x.shape[:-1] + (pad,))], dim=-1) if pad else x


def as_features_scene(sc, feat, g_all):
    """scene sc (render_ref64._scene's fields) with feat [V, C] in place of its colour and background 0;
    g_all [H, W, C + 1] = [g_F | g_alpha]"""
    d = SimpleNamespace(**vars(sc))
    d.feat = feat.detach().float().cpu().contiguous()
    d.C = int(d.feat.shape[1])
    d.g_all = g_all.detach().float().cpu().contiguous()
    chan = torch.cat([d.feat.double(), torch.ones(sc.V, 1, dtype=torch.float64)], dim=1)
    d.coeff64_all = _padded(chan, d.C) / Y0               # [V, 3 G]
    d.bg = torch.zeros(3)
    return d


def group_scene(sc, j):
    """the scene of group j as render_fp64 / oracle_run take it"""
    d = SimpleNamespace(**vars(sc))
    d.coeff64 = sc.coeff64_all[:, 3 * j:3 * j + 3].contiguous()
    d.coeff16 = d.coeff64.float().reshape(-1, 3, 1).contiguous()   # what render_ref64.scene_coeff hands the oracle
    return d


@functools.lru_cache(maxsize=None)
def features_scene(name, C):
    scenes = R.render_scenes()
    sc = scenes[name]
    gen = torch.Generator().manual_seed(7000 + 64 * list(scenes).index(name) + C)
    feat = torch.randn(sc.V, C, generator=gen)
    g_all = torch.randn(sc.H, sc.W, C + 1, generator=gen)
    return as_features_scene(sc, feat, g_all)


def combine(groups, C):
    """per-group render results (dicts in render_ref64's naming: image and / or the four gradients) -> feature_map,
    alpha and the gradients re-keyed to KEYS; float64"""
    res = {}
    if "image" in groups[0]:
        maps = torch.cat([g["image"].double() for g in groups], dim=2)
        res.update(feature_map=maps[..., :C], alpha=maps[..., C])
    if "g_rgb" in groups[0]:
        rows = torch.cat([g["g_rgb"].double().reshape(g["g_rgb"].shape[0], 3) for g in groups], dim=1) / Y0
        res["g_features"] = rows[:, :C]
        for k in SHARED:
            res[k] = sum(g[k].double() for g in groups)
    return res


def reference_of(sc, g_all):
    """render_fp64 (FP32 settings) of features scene sc for g_all [H, W, C + 1], group by group -> a namespace with
    feature_map [H, W, C], alpha [H, W], fragile / nsp / scale / used and grad / grad_walk / abs / abs_walk keyed by
    KEYS, plus grad_image [H, W, C + 1] (g_all, zero on the fragile pixels)"""
    C = sc.C
    gp = _padded(g_all.detach().float().cpu(), C)
    outs = []
    for j in range(n_groups(C)):
        outs.append(R.render_fp64(sc.uv, sc.opacity, sc.coeff64_all[:, 3 * j:3 * j + 3], sc.conic, sc.rays, sc.ranges,
                                  sc.sorted_g, sc.bg, sc.W, sc.H, R.FP32, gp[..., 3 * j:3 * j + 3]))
    first = outs[0]
    for o in outs[1:]:   # the decisions do not depend on the channels
        assert torch.equal(o.fragile, first.fragile) and torch.equal(o.nsp, first.nsp) and torch.equal(o.scale, first.scale)
    ref = SimpleNamespace(fragile=first.fragile, nsp=first.nsp, scale=first.scale, C=C)
    ref.used = torch.stack([o.used for o in outs]).any(dim=0)
    ref.grad_image = (g_all.double() * (~ref.fragile)[:, :, None]).contiguous()
    fwd = combine([dict(image=o.image) for o in outs], C)
    ref.feature_map, ref.alpha = fwd["feature_map"], fwd["alpha"]
    for k in ("grad", "grad_walk", "abs", "abs_walk"):
        setattr(ref, k, combine([getattr(o, k) for o in outs], C))
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, C, unscaled_only=False):
    """the reference of scene `name` with C channels; unscaled_only: the gradients are zero on the pixels whose walk
    gradient is scaled too (there the fp32 oracle's gradient is the true derivative).  Computed once; do not modify."""
    sc = features_scene(name, C)
    g_all = sc.g_all
    if unscaled_only:
        g_all = g_all * (reference(name, C).scale == 1)[:, :, None]
    return reference_of(sc, g_all)


def oracle_of(sc, grad_image, oracle_run):
    """the fp32 oracle (tests/test_render_ref64.oracle_run, exact walk) group by group on grad_image [H, W, C + 1],
    combined as the reference is -> dict feature_map, alpha, nsp and KEYS"""
    C = sc.C
    gp = _padded(grad_image.float(), C)
    outs = [oracle_run(group_scene(sc, j), 1, torch.float32, gp[..., 3 * j:3 * j + 3].contiguous(), exact=True)
            for j in range(n_groups(C))]
    res = combine(outs, C)
    res["nsp"] = outs[0]["nsp"]
    return res
