"""The reference of the depth-distortion map (gs_render_distortion, fused.rasterize_distortion): plain float64, written
from the formulas with torch autograd in the style of tests/render_ref64.py (test code only).

Per tile, [pixels, list entries] tensors.  alpha, the contribute and the stop decision are render_ref64's under its FP32
settings (the same formulas; num_splats is asserted equal to render_fp64's, whose `fragile` mask is the one used here).
With w_k = alpha_k T_k over the contributors, z the scene's camera-frame depth, in LIST order:

  A_<k = sum_{j<k} w_j      D_<k = sum_{j<k} w_j z_j
  distortion = 2 sum_k w_k (z_k A_<k - D_<k)      depth = sum w_k z_k      alpha = sum w_k

The scenes are depth_alpha_ref.depth_scene(name) with their seeded z as they are -- NOT list-sorted: the list-order form
is the definition the kernels are held to; on z-sorted lists it is sum_{i,j} w_i w_j |z_i - z_j| (pairwise() below).
(g_dist, g_depth, g_alpha) are the three channels of the scene's grad_image (render_scenes()'s, all three), zero on
the fragile pixels.  `grad` is the derivative with the decisions held constant, from autograd.

`abs`: per gradient element the float64 sum of the magnitudes of the leaf terms of its formula, as
render_ref64._abs_sums.  With e_k = d distortion / d w_k = 2 [z_k (A_<k - A_>k) - D_<k + D_>k] the magnitudes per channel
  m_dist,k = 2 (|z_k| (A_<k + A_>k) + sum_{j != k} w_j |z_j|)      m_depth,k = |z_k|      m_alpha,k = 1
enter dL/dalpha_k = T_k c_k - S_k / (1 - alpha_k) as sum_ch |g_ch| (T_k m_ch,k + sum_{j>k} w_j m_ch,j / (1 - alpha_k)),
then the chain to opacity, uv, conic with _abs_sums' factors; dL/dz_k has |g_depth| w_k + |g_dist| 2 w_k (A_<k + A_>k).
abs_p [H, W] is the same for the forward: 2 sum_k w_k (|z_k| A_<k + sum_{j<k} w_j |z_j|).

`rest`: the fp32 restatement -- the same sequential recurrences evaluated in float32 on the CPU, vectorised over the
pixels of a tile, one step per list entry, with the reference's decisions.  Forward
  X = X + w (z A - D),  D = D + w z,  A = A + w,  T = T - alpha T;
backward from T_end back to front with T_k = T / (1 - alpha_k), the suffix sums A_>k, D_>k and the prefixes as totals
minus suffix minus the entry's own term, then the chain in float32.  It is one valid fp32 evaluation: its distance from
the reference is the yardstick the kernels' distance is held against."""
import functools
from types import SimpleNamespace

import torch

from . import depth_alpha_ref as D
from . import render_ref64 as R
from .test_gpu_render_ref64 import noise_measure   # noqa: F401 (re-exported)

KEYS = D.KEYS   # g_z, g_opacity, g_uv, g_conic
ST = R.FP32


def _geometry(uv, opacity, conic, idx, px, py, dtype):
    """the per (pixel, entry) quantities of render_ref64's formulas in `dtype`"""
    dx = px.to(dtype)[:, None] - uv[idx, 0][None, :]
    dy = py.to(dtype)[:, None] - uv[idx, 1][None, :]
    a = (conic[idx, 0] + ST.blur)[None, :]
    b = (conic[idx, 1] / 2)[None, :]
    c = (conic[idx, 2] + ST.blur)[None, :]
    det = a * c - b * b
    q = c * dx * dx - 2 * b * dx * dy + a * dy * dy
    m = q / det
    prob = torch.exp(-m / 2)
    opa = opacity[idx, 0][None, :]
    alpha = torch.where(m > 0, opa * prob, torch.zeros_like(m))
    return SimpleNamespace(dx=dx, dy=dy, a=a, b=b, c=c, det=det, q=q, m=m, prob=prob, opa=opa, alpha=alpha)


def _tiles(sc):
    ntx, nty = (sc.W + 15) // 16, (sc.H + 15) // 16
    for ty in range(nty):
        for tx in range(ntx):
            tile = ty * ntx + tx
            idx = sc.sorted_g[int(sc.ranges[tile]):int(sc.ranges[tile + 1])].long()
            px, py = R._tile_pixels(tx, ty, sc.W, sc.H)
            yield tile, idx, px, py


def decisions_of(sc):
    """per tile with a non-empty list: contrib [P, L] bool and the entries walked [P], from the fp32 values of the
    inputs in float64, as render_fp64 takes them"""
    out = {}
    uv, opacity, conic = sc.uv.double(), sc.opacity.double(), sc.conic.double()
    for tile, idx, px, py in _tiles(sc):
        if idx.numel() == 0:
            continue
        g = _geometry(uv, opacity, conic, idx, px, py, torch.float64)
        cand = g.alpha >= ST.alpha_min
        T_incl = torch.cumprod(1 - g.alpha * cand, dim=1)
        T = torch.cat([torch.ones(px.numel(), 1, dtype=torch.float64), T_incl[:, :-1]], dim=1)
        walked = (1 - T) <= R.SAT
        if bool((cand & walked & (g.alpha > R.ALPHA_MAX)).any()):
            raise ValueError("a contributing alpha exceeds 0.99: outside what the reference models")
        out[tile] = (cand & walked, walked.sum(dim=1))
    return out


def _excl(x):
    """exclusive prefix sum along the list"""
    return torch.cumsum(x, dim=1) - x


def composite(sc, uv, opacity, conic, z, decisions):
    """float64 maps (distortion, depth, alpha, T_end) [H, W] of the scene for the given leaves (autograd flows),
    the decisions held as given"""
    H, W = sc.H, sc.W
    maps = [torch.zeros(H, W, dtype=torch.float64) for _ in range(3)] + [torch.ones(H, W, dtype=torch.float64)]
    pieces = []
    for tile, idx, px, py in _tiles(sc):
        if idx.numel() == 0:
            continue
        contrib = decisions[tile][0]
        g = _geometry(uv, opacity, conic, idx, px, py, torch.float64)
        one_minus = torch.where(contrib, 1 - g.alpha, torch.ones_like(g.alpha))
        T_incl = torch.cumprod(one_minus, dim=1)
        T = torch.cat([torch.ones(px.numel(), 1, dtype=torch.float64), T_incl[:, :-1]], dim=1)
        w = g.alpha * T * contrib
        zk = z[idx][None, :]
        wz = w * zk
        dist = 2 * (w * (zk * _excl(w) - _excl(wz))).sum(dim=1)
        pieces.append((px, py, dist, wz.sum(dim=1), w.sum(dim=1), T_incl[:, -1]))
    for i in range(4):
        if pieces:
            maps[i] = maps[i].index_put((torch.cat([p[1] for p in pieces]), torch.cat([p[0] for p in pieces])),
                                        torch.cat([p[2 + i] for p in pieces]))
    return maps


def pairwise(sc, decisions, z=None):
    """[H, W] float64: sum_{i,j} w_i w_j |z_i - z_j| over each pixel's contributors, formed as the double sum"""
    z = (sc.z if z is None else z).double()
    uv, opacity, conic = sc.uv.double(), sc.opacity.double(), sc.conic.double()
    out = torch.zeros(sc.H, sc.W, dtype=torch.float64)
    for tile, idx, px, py in _tiles(sc):
        if idx.numel() == 0:
            continue
        contrib = decisions[tile][0]
        g = _geometry(uv, opacity, conic, idx, px, py, torch.float64)
        one_minus = torch.where(contrib, 1 - g.alpha, torch.ones_like(g.alpha))
        T_incl = torch.cumprod(one_minus, dim=1)
        T = torch.cat([torch.ones(px.numel(), 1, dtype=torch.float64), T_incl[:, :-1]], dim=1)
        w = g.alpha * T
        for p in range(px.numel()):
            sel = contrib[p]
            wp, zp = w[p][sel], z[idx][sel]
            out[py[p], px[p]] = (wp[:, None] * wp[None, :] * (zp[:, None] - zp[None, :]).abs()).sum()
    return out


def _chain_abs(acc, idx, g, ga):
    """render_ref64._abs_sums' chain from the magnitude ga of dL/dalpha [P, L] to opacity, uv and conic"""
    acc["g_opacity"].index_add_(0, idx, (g.prob * ga).sum(dim=0)[:, None])
    gm = 0.5 * g.prob * g.opa.abs() * ga
    rd = 1 / g.det
    dx, dy, a, b, c = g.dx, g.dy, g.a, g.b, g.c
    qa = (a.abs() * dy * dy + 2 * (b * dx * dy).abs() + c.abs() * dx * dx) * rd * rd
    acc["g_uv"].index_add_(0, idx, torch.stack([((2 * (c * dx).abs() + 2 * (b * dy).abs()) * rd * gm).sum(dim=0),
                                                ((2 * (a * dy).abs() + 2 * (b * dx).abs()) * rd * gm).sum(dim=0)], dim=1))
    acc["g_conic"].index_add_(0, idx, torch.stack([((dy * dy * rd + c.abs() * qa) * gm).sum(dim=0),
                                                   (((dx * dy).abs() * rd + b.abs() * qa) * gm).sum(dim=0),
                                                   ((dx * dx * rd + a.abs() * qa) * gm).sum(dim=0)], dim=1))


def _abs_sums(sc, decisions, gi):
    """-> (abs dict over KEYS, abs_p [H, W]) for grad_image gi [H, W, 3] = (g_dist, g_depth, g_alpha), float64"""
    V = sc.V
    uv, opacity, conic, z = sc.uv.double(), sc.opacity.double(), sc.conic.double(), sc.z.double()
    acc = dict(g_z=torch.zeros(V, dtype=torch.float64), g_opacity=torch.zeros(V, 1, dtype=torch.float64),
               g_uv=torch.zeros(V, 2, dtype=torch.float64), g_conic=torch.zeros(V, 3, dtype=torch.float64))
    abs_p = torch.zeros(sc.H, sc.W, dtype=torch.float64)
    for tile, idx, px, py in _tiles(sc):
        if idx.numel() == 0:
            continue
        contrib = decisions[tile][0]
        g = _geometry(uv, opacity, conic, idx, px, py, torch.float64)
        one_minus = torch.where(contrib, 1 - g.alpha, torch.ones_like(g.alpha))
        T_incl = torch.cumprod(one_minus, dim=1)
        T = torch.cat([torch.ones(px.numel(), 1, dtype=torch.float64), T_incl[:, :-1]], dim=1) * contrib
        w = g.alpha * T
        za = z[idx].abs()[None, :]
        wza = w * za
        A_lt, Z_lt = _excl(w), _excl(wza)
        A_all, Z_all = w.sum(dim=1, keepdim=True), wza.sum(dim=1, keepdim=True)
        A_gt = A_all - A_lt - w
        abs_p[py, px] = 2 * (w * (za * A_lt + Z_lt)).sum(dim=1)
        agi = gi[py, px].abs()
        mags = (2 * (za * (A_lt + A_gt) + Z_all - wza), za.expand_as(w), torch.ones_like(w))
        ga = torch.zeros_like(w)
        for ch, mag in enumerate(mags):
            wm = w * mag
            behind = wm.sum(dim=1, keepdim=True) - torch.cumsum(wm, dim=1)
            ga = ga + agi[:, ch][:, None] * (T * mag + behind / (1 - g.alpha))
        ga = ga * contrib
        acc["g_z"].index_add_(0, idx, (agi[:, 1][:, None] * w + agi[:, 0][:, None] * 2 * w * (A_lt + A_gt)).sum(dim=0))
        _chain_abs(acc, idx, g, ga)
    return acc, abs_p


def restatement(sc, decisions, gi):
    """the fp32 restatement (module docstring) -> dict of float32 tensors: distortion, depth, alpha, t_end [H, W] and
    g_z [V], g_opacity [V, 1], g_uv [V, 2], g_conic [V, 3] for grad_image gi [H, W, 3]"""
    f32 = torch.float32
    V, H, W = sc.V, sc.H, sc.W
    uv, opacity, conic, z = sc.uv.float(), sc.opacity.float(), sc.conic.float(), sc.z.float()
    gi = gi.float()
    out = dict(distortion=torch.zeros(H, W), depth=torch.zeros(H, W), alpha=torch.zeros(H, W), t_end=torch.ones(H, W),
               g_z=torch.zeros(V), g_opacity=torch.zeros(V, 1), g_uv=torch.zeros(V, 2), g_conic=torch.zeros(V, 3))
    for tile, idx, px, py in _tiles(sc):
        if idx.numel() == 0:
            continue
        contrib = decisions[tile][0]
        g = _geometry(uv, opacity, conic, idx, px, py, f32)
        P, L = contrib.shape
        zk = z[idx]
        X, Dm, A, T = torch.zeros(P), torch.zeros(P), torch.zeros(P), torch.ones(P)
        for k in range(L):
            on = contrib[:, k]
            if not bool(on.any()):
                continue
            al = g.alpha[:, k]
            w = al * T
            X = torch.where(on, X + w * (zk[k] * A - Dm), X)
            Dm = torch.where(on, Dm + w * zk[k], Dm)
            A = torch.where(on, A + w, A)
            T = torch.where(on, T - al * T, T)
        out["distortion"][py, px], out["depth"][py, px], out["alpha"][py, px], out["t_end"][py, px] = 2 * X, Dm, A, T
        gx, gd, ga = (gi[py, px][:, i] for i in range(3))
        S, A_gt, D_gt = torch.zeros(P), torch.zeros(P), torch.zeros(P)
        dalpha = torch.zeros(P, L)
        gz = torch.zeros(P, L)
        for k in range(L - 1, -1, -1):
            on = contrib[:, k]
            if not bool(on.any()):
                continue
            al = g.alpha[:, k]
            r1ma = 1 / (1 - al)
            Tk = T * r1ma
            w = al * Tk
            wz = w * zk[k]
            A_lt = A - A_gt - w
            D_lt = Dm - D_gt - wz
            dA = A_lt - A_gt
            e = 2 * (zk[k] * dA - D_lt + D_gt)
            c = gx * e + (gd * zk[k] + ga)
            dalpha[:, k] = torch.where(on, Tk * c - S * r1ma, dalpha[:, k])
            gz[:, k] = torch.where(on, gd * w + gx * (2 * w * dA), gz[:, k])
            S = torch.where(on, S + w * c, S)
            A_gt = torch.where(on, A_gt + w, A_gt)
            D_gt = torch.where(on, D_gt + wz, D_gt)
            T = torch.where(on, Tk, T)
        out["g_z"].index_add_(0, idx, gz.sum(dim=0))
        out["g_opacity"].index_add_(0, idx, (g.prob * dalpha).sum(dim=0)[:, None])
        gm = -0.5 * g.alpha * dalpha   # dL/dm
        rd = 1 / g.det
        dx, dy, a, b, c = g.dx, g.dy, g.a, g.b, g.c
        qd = g.q * rd * rd
        out["g_uv"].index_add_(0, idx, torch.stack([(-(2 * c * dx - 2 * b * dy) * rd * gm).sum(dim=0),
                                                    (-(2 * a * dy - 2 * b * dx) * rd * gm).sum(dim=0)], dim=1))
        out["g_conic"].index_add_(0, idx, torch.stack([((dy * dy * rd - c * qd) * gm).sum(dim=0),
                                                       ((-dx * dy * rd + b * qd) * gm).sum(dim=0),
                                                       ((dx * dx * rd - a * qd) * gm).sum(dim=0)], dim=1))
    return out


def reference_of(sc, grad_image, fragile, nsp=None, with_restatement=True):
    """depth scene sc (depth_alpha_ref.as_depth_scene's fields), grad_image [H, W, 3] = (g_dist, g_depth, g_alpha),
    fragile [H, W] (render_fp64's, FP32 settings; nsp: its num_splats, asserted equal to the walk here) ->
    SimpleNamespace(distortion, depth, alpha, t_end, abs_p [H, W] float64; nsp; fragile; grad_image (zero on fragile
    pixels); grad / abs (dicts over KEYS); used [V]; decisions; rest (the fp32 restatement))"""
    decisions = decisions_of(sc)
    my_nsp = torch.zeros(sc.H, sc.W, dtype=torch.int32)
    for tile, idx, px, py in _tiles(sc):
        if idx.numel():
            my_nsp[py, px] = decisions[tile][1].int()
    if nsp is not None:
        assert torch.equal(my_nsp, nsp), "the decisions differ from render_fp64's"
    gi = (grad_image.detach().double() * (~fragile)[:, :, None]).contiguous()
    leaf = lambda x: x.detach().double().clone().requires_grad_(True)
    uv, opacity, conic, z = leaf(sc.uv), leaf(sc.opacity), leaf(sc.conic), leaf(sc.z)
    dist, depth, alpha, t_end = composite(sc, uv, opacity, conic, z, decisions)
    loss = (dist * gi[..., 0] + depth * gi[..., 1] + alpha * gi[..., 2]).sum()
    if loss.requires_grad:
        g = torch.autograd.grad(loss, (z, opacity, uv, conic), allow_unused=True)
    else:
        g = (None,) * 4
    grad = {k: (torch.zeros_like(x) if gr is None else gr.detach()) for k, x, gr in zip(KEYS, (z, opacity, uv, conic), g)}
    ab, abs_p = _abs_sums(sc, decisions, gi)
    used = torch.zeros(sc.V, dtype=torch.bool)
    for tile, idx, px, py in _tiles(sc):
        if idx.numel():
            live = decisions[tile][0] & (gi[py, px].abs().sum(dim=1) > 0)[:, None]
            used[idx[live.any(dim=0)]] = True
    return SimpleNamespace(distortion=dist.detach(), depth=depth.detach(), alpha=alpha.detach(), t_end=t_end.detach(),
                           abs_p=abs_p, nsp=my_nsp, fragile=fragile, grad_image=gi, grad=grad, abs=ab, used=used,
                           decisions=decisions, rest=restatement(sc, decisions, gi) if with_restatement else None)


def scene_grad_image(name):
    """(g_dist, g_depth, g_alpha): the three channels of the scene's grad_image"""
    return R.render_scenes()[name].grad_image


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reference of depth scene `name`.  Computed once; do not modify."""
    base = D.reference(name)
    return reference_of(D.depth_scene(name), scene_grad_image(name), base.fragile, base.nsp)


def forward_ratio(got, ref, ok):
    """max over the pixels `ok` of |got - ref| / (|restatement - ref| + 2^-24 abs_p + 2^-22 |ref|) (0 where got == ref)"""
    num = (got.double() - ref.distortion).abs()[ok]
    den = ((ref.rest["distortion"].double() - ref.distortion).abs() + 2.0 ** -24 * ref.abs_p
           + 2.0 ** -22 * ref.distortion.abs())[ok]
    r = torch.where(num == 0, torch.zeros_like(num), num / den)
    return float(r.max()) if r.numel() else 0.0
