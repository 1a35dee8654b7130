"""A float64 reference of the per-Gaussian contribution statistics (gs_render_contributions,
fused.rasterize_contributions), test code only.

Written from the formulas in the docstring of tests/render_ref64.py, not from csrc/render.hip.  Per tile it forms
[pixels, list entries] tensors with the FP32 settings of that module (blur 0.25, alpha_min, the walk stops before the
first entry at which A exceeds 0.9999, alpha = 0 unless m > 0):

  d = (px - u, py - v),  a, b, c = conic0 + blur, conic1 / 2, conic2 + blur,  m = (c dx^2 - 2 b dx dy + a dy^2) / (a c - b^2)
  alpha = opacity exp(-m / 2) if m > 0 else 0;  contributes iff alpha >= alpha_min and the pixel's walk reached the entry
  T = prod over the contributing entries in front of (1 - alpha),  w = alpha T

and reduces w over the PIXELS per Gaussian g (over every tile that lists g):

  weight_sum[g] = sum w      weight_max[g] = max w      pixel_count[g] = number of contributing (pixel, entry) pairs

nsp [H, W] counts the entries a pixel walked.  fragile [H, W] marks the pixels with a decision within the relative
margin MARGIN (render_ref64's) of its threshold: a walked alpha near alpha_min, a prefix A (the final one included) near
0.9999, the final A near 0.999, a walked m != 0 with |m| <= MARGIN.

The same formulas are evaluated a second time in torch.float32 on the fp32 inputs, with the float64 run's decisions
(which entries are walked and which contribute): env_sum / env_max = |that - the float64 value| per Gaussian, the error
the formulas' own fp32 arithmetic makes, which is what ref64.r_measure takes as its envelope."""
import functools
from types import SimpleNamespace

import torch

from . import render_ref64 as R


def _tile_weights(px, py, uv, opacity, conic, idx, dtype, decisions=None):
    """[P, L] alpha, m, T (in front of each entry) and w of one tile in `dtype`; decisions = (walked, contrib) of an
    earlier evaluation, or None to take them here"""
    st = R.FP32
    uv, o, cn = uv.to(dtype), opacity.to(dtype).reshape(-1), conic.to(dtype)
    dx = px.to(dtype)[:, None] - uv[idx, 0][None, :]
    dy = py.to(dtype)[:, None] - uv[idx, 1][None, :]
    blur = torch.tensor(st.blur, dtype=dtype)
    a = (cn[idx, 0] + blur)[None, :]
    b = (cn[idx, 1] / 2)[None, :]
    c = (cn[idx, 2] + blur)[None, :]
    m = (c * dx * dx - 2 * b * dx * dy + a * dy * dy) / (a * c - b * b)
    alpha = torch.where(m > 0, o[idx][None, :] * torch.exp(-m / 2), torch.zeros_like(m))
    P = px.numel()
    if decisions is None:
        cand = alpha >= st.alpha_min
    else:
        cand = decisions[1]   # (beyond the walk nobody contributes: T there is not used)
    one_minus = 1 - alpha * cand
    T = torch.cat([torch.ones(P, 1, dtype=dtype), torch.cumprod(one_minus, dim=1)[:, :-1]], dim=1)
    if decisions is None:
        walked = (1 - T) <= R.SAT          # A is monotone: the walk is a prefix of the list
        contrib = cand & walked
    else:
        walked, contrib = decisions
    w = alpha * T * contrib
    return SimpleNamespace(alpha=alpha, m=m, T=T, w=w, walked=walked, contrib=contrib, cand=cand)


def _fragile(t, margin):
    st = R.FP32
    near_min = (t.walked & ((t.alpha - st.alpha_min).abs() <= margin * st.alpha_min)).any(dim=1)
    A = torch.where(t.walked, 1 - t.T, torch.zeros_like(t.T))
    A_final = 1 - torch.where(t.contrib, 1 - t.alpha, torch.ones_like(t.alpha)).prod(dim=1)
    A_all = torch.cat([A, A_final[:, None]], dim=1)
    near_sat = ((A_all - R.SAT).abs() <= margin * R.SAT).any(dim=1)
    near_bg = (A_final - R.BG_BELOW).abs() <= margin * R.BG_BELOW
    near_zero = (t.walked & (t.m != 0) & (t.m.abs() <= margin)).any(dim=1)
    return near_min | near_sat | near_bg | near_zero


def contributions(uv, opacity, conic, ranges, sorted_g, W, H, margin=R.MARGIN, walk=None):
    """uv [V,2], opacity [V] or [V,1], conic [V,3] (fp32 values), ranges [tiles+1], sorted_g [S] ->
    SimpleNamespace(weight_sum, weight_max [V] float64, pixel_count [V] int64, env_sum, env_max [V] float64,
    nsp [H,W] int32, fragile [H,W] bool, skipped: walked visits with 0 < alpha < alpha_min, tiles_of [V]: tiles listing g)
    walk [H,W] (optional): the number of entries each pixel walks is GIVEN (the colour forward's num_splats_per_pixel,
    an input of the statistics kernel) instead of decided here; nsp and fragile are still this reference's own"""
    uv, opacity, conic = (x.detach().cpu().float() for x in (uv, opacity, conic))
    V = uv.shape[0]
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    f64 = dict(dtype=torch.float64)
    wsum, wmax = torch.zeros(V, **f64), torch.zeros(V, **f64)
    wsum32, wmax32 = torch.zeros(V), torch.zeros(V)
    count = torch.zeros(V, dtype=torch.int64)
    tiles_of = torch.zeros(V, dtype=torch.int64)
    nsp = torch.zeros(H, W, dtype=torch.int32)
    fragile = torch.zeros(H, W, dtype=torch.bool)
    skipped = 0
    for ty in range(nty):
        for tx in range(ntx):
            tile = ty * ntx + tx
            idx = sorted_g[int(ranges[tile]):int(ranges[tile + 1])].long().cpu()
            if idx.numel() == 0:
                continue
            px, py = R._tile_pixels(tx, ty, W, H)
            t = _tile_weights(px, py, uv, opacity, conic, idx, torch.float64)
            nsp[py, px] = t.walked.sum(dim=1).int()
            fragile[py, px] = _fragile(t, margin)
            if walk is not None:
                walked = torch.arange(idx.numel())[None, :] < walk[py, px].long()[:, None]
                t = _tile_weights(px, py, uv, opacity, conic, idx, torch.float64, (walked, t.cand & walked))
                t.cand = t.alpha >= R.FP32.alpha_min
            t32 = _tile_weights(px, py, uv, opacity, conic, idx, torch.float32, (t.walked, t.contrib))
            # a Gaussian is listed once per tile: plain indexed updates
            wsum[idx] += t.w.sum(dim=0)
            wmax[idx] = torch.maximum(wmax[idx], t.w.amax(dim=0))
            wsum32[idx] += t32.w.sum(dim=0)
            wmax32[idx] = torch.maximum(wmax32[idx], t32.w.amax(dim=0))
            count[idx] += t.contrib.sum(dim=0)
            tiles_of[idx] += 1
            skipped += int((t.walked & (t.alpha > 0) & ~t.cand).sum())
    return SimpleNamespace(weight_sum=wsum, weight_max=wmax, pixel_count=count, env_sum=(wsum32.double() - wsum).abs(),
                           env_max=(wmax32.double() - wmax).abs(), nsp=nsp, fragile=fragile, skipped=skipped,
                           tiles_of=tiles_of)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the statistics of scene `name` of render_ref64.render_scenes().  Computed once; do not modify."""
    sc = R.render_scenes()[name]
    return contributions(sc.uv, sc.opacity, sc.conic, sc.ranges, sc.sorted_g, sc.W, sc.H)
