"""The reference of the median-depth map (gs_render_median_depth, fused.rasterize_median_depth): plain
float64, per tile, in the style of tests/distortion_ref.py, whose restatement of render_ref64.render_fp64's alpha /
contribute / stop expressions under the FP32 settings is the one used here (test code only).

Per tile, [pixels, list entries] tensors.  With T_k the transmittance in front of entry k (the product of 1 - alpha_j
over the contributors j < k, in LIST order), the median entry of a pixel is its LAST contributing entry with T_k > 0.5:

  median_index = that entry's Gaussian (-1: no contributor)      median_depth = its z (0 with -1)
  grad_z = index_add(grad_median by median_index)                (the choice held constant; nothing else gets a gradient)

The scenes are depth_alpha_ref.depth_scene(name) with their seeded z as they are -- NOT list-sorted: the list-order form
is the definition the kernels are held to.

median_closeness [H, W] = min over the contributing k of |T_k - 0.5| / 0.5: how near the pixel's strict comparison
T_k > 0.5 comes to flipping.  A pixel is MEDIAN-FRAGILE where that is <= MEDIAN_MARGIN; grad_median is zeroed there and
on render_ref64's fragile pixels (where a contribute / stop decision may flip).

MEDIAN_MARGIN = 2^-17 was not measured on the kernels.  On the CPU, on the eight render_scenes(), a float32 evaluation of
the same expressions (restatement() below: torch float32, T <- fma(-alpha, T, T) entry by entry) departs from float64 by
at most 8.8e-7 relative in any T_k up to the median entry (long_1100; 7.7e-7 on faint_300, 3.0e-7 at most elsewhere)
and takes the same median decision on every pixel; 2^-17 = 7.6e-6 is more than eight times that, which leaves room for
the kernels' own exponential.
tests/test_median_depth_ref.py keeps both statements measured (deviation <= MEDIAN_MARGIN / 8) and holds the share of
median-fragile pixels under 1 % per scene.

`rest`: the fp32 restatement -- the same recurrence in float32 on the CPU with the reference's contribute decisions:
its own median choice, T_k, and grad_z as a float32 index_add.  It is one valid fp32 evaluation: its distance from the
reference is the yardstick the kernels' distance is held against."""
import functools
from types import SimpleNamespace

import torch

from . import depth_alpha_ref as D
from . import distortion_ref as X
from . import render_ref64 as R

MEDIAN_MARGIN = 2.0 ** -17


def _walk64(sc, decisions):
    """per tile with a non-empty list -> SimpleNamespace(idx [L], px, py [P], contrib [P, L] bool, T [P, L] in front of
    each entry, T_behind [P, L], alpha [P, L], j [P] the median entry's list position (-1: no contributor),
    j_last [P] the last contributor's)"""
    uv, opacity, conic = sc.uv.double(), sc.opacity.double(), sc.conic.double()
    out = {}
    for tile, idx, px, py in X._tiles(sc):
        if idx.numel() == 0:
            continue
        contrib = decisions[tile][0]
        g = X._geometry(uv, opacity, conic, idx, px, py, torch.float64)
        one_minus = torch.where(contrib, 1 - g.alpha, torch.ones_like(g.alpha))
        T_behind = torch.cumprod(one_minus, dim=1)
        T = torch.cat([torch.ones(px.numel(), 1, dtype=torch.float64), T_behind[:, :-1]], dim=1)
        pos = torch.arange(idx.numel())[None, :]
        none = torch.full_like(pos, -1)
        j = torch.where(contrib & (T > 0.5), pos, none).amax(dim=1)
        j_last = torch.where(contrib, pos, none).amax(dim=1)
        out[tile] = SimpleNamespace(idx=idx, px=px, py=py, contrib=contrib, T=T, T_behind=T_behind, alpha=g.alpha, j=j,
                                    j_last=j_last)
    return out


def _pick(idx, j):
    """the Gaussian of list position j [P] (-1 stays -1)"""
    return torch.where(j >= 0, idx[j.clamp(min=0)], torch.full_like(j, -1))


def restatement(sc, decisions, walk, grad_median):
    """the fp32 restatement (module docstring) -> SimpleNamespace(index [H, W] int64, g_z [V] float32 for grad_median
    [H, W] scattered by ITS index, t_deviation: the largest |T_k32 - T_k| / T_k over the contributing entries up to the
    reference's median entry)"""
    f32 = torch.float32
    uv, opacity, conic = sc.uv.float(), sc.opacity.float(), sc.conic.float()
    index = torch.full((sc.H, sc.W), -1, dtype=torch.int64)
    dev = 0.0
    for tile, idx, px, py in X._tiles(sc):
        if idx.numel() == 0:
            continue
        contrib = decisions[tile][0]
        w = walk[tile]
        g = X._geometry(uv, opacity, conic, idx, px, py, f32)
        P, L = contrib.shape
        T = torch.ones(P)
        j = torch.full((P,), -1, dtype=torch.int64)
        Tk = torch.ones(P, L)
        for k in range(L):
            on = contrib[:, k]
            Tk[:, k] = T
            if not bool(on.any()):
                continue
            j = torch.where(on & (T > 0.5), torch.full_like(j, k), j)
            # fma(-alpha, T, T): the product of two floats is exact in float64, the sum rounds once more to float32
            T = torch.where(on, (T.double() - g.alpha[:, k].double() * T.double()).float(), T)
        index[py, px] = _pick(idx, j)
        upto = contrib & (torch.arange(L)[None, :] <= w.j[:, None])
        if bool(upto.any()):
            dev = max(dev, float(((Tk.double() - w.T).abs() / w.T)[upto].max()))
    g_z = torch.zeros(sc.V)
    sel = index >= 0
    g_z.index_add_(0, index[sel], grad_median.float()[sel])
    return SimpleNamespace(index=index, g_z=g_z, t_deviation=dev)


def reference_of(sc, grad_median, fragile, nsp=None, with_restatement=True):
    """depth scene sc (depth_alpha_ref.as_depth_scene's fields), grad_median [H, W], fragile [H, W] (render_fp64's, FP32
    settings; nsp: its num_splats, asserted equal to the walk here) -> SimpleNamespace(median_index [H, W] int64,
    median_depth, depth, alpha, median_closeness [H, W] float64; median_fragile, fragile, ok (neither) [H, W] bool; nsp;
    grad_median (zero outside ok); grad_z, abs_z [V] float64 (the index_add and the index_add of the magnitudes);
    used [V]; decisions; walk (per tile, _walk64's); rest (the fp32 restatement))"""
    decisions = X.decisions_of(sc)
    walk = _walk64(sc, decisions)
    H, W = sc.H, sc.W
    z = sc.z.double()
    index = torch.full((H, W), -1, dtype=torch.int64)
    close = torch.full((H, W), float("inf"), dtype=torch.float64)
    depth, alpha = torch.zeros(H, W, dtype=torch.float64), torch.zeros(H, W, dtype=torch.float64)
    my_nsp = torch.zeros(H, W, dtype=torch.int32)
    for tile, w in walk.items():
        index[w.py, w.px] = _pick(w.idx, w.j)
        inf = torch.full_like(w.T, float("inf"))
        close[w.py, w.px] = torch.where(w.contrib, (w.T - 0.5).abs() / 0.5, inf).amin(dim=1)
        wgt = w.alpha * w.T * w.contrib
        depth[w.py, w.px] = (wgt * z[w.idx][None, :]).sum(dim=1)
        alpha[w.py, w.px] = wgt.sum(dim=1)
        my_nsp[w.py, w.px] = decisions[tile][1].int()
    if nsp is not None:
        assert torch.equal(my_nsp, nsp), "the decisions differ from render_fp64's"
    sel = index >= 0
    median_depth = torch.where(sel, z[index.clamp(min=0)], torch.zeros(H, W, dtype=torch.float64))
    median_fragile = close <= MEDIAN_MARGIN
    ok = ~(fragile | median_fragile)
    gm = (grad_median.detach().double() * ok).contiguous()
    grad_z = torch.zeros(sc.V, dtype=torch.float64).index_add_(0, index[sel], gm[sel])
    abs_z = torch.zeros(sc.V, dtype=torch.float64).index_add_(0, index[sel], gm[sel].abs())
    used = torch.zeros(sc.V, dtype=torch.bool)
    used[index[sel & (gm != 0)]] = True
    return SimpleNamespace(median_index=index, median_depth=median_depth, depth=depth, alpha=alpha,
                           median_closeness=close, median_fragile=median_fragile, fragile=fragile, ok=ok, nsp=my_nsp,
                           grad_median=gm, grad_z=grad_z, abs_z=abs_z, used=used, decisions=decisions, walk=walk,
                           rest=restatement(sc, decisions, walk, gm) if with_restatement else None)


def choice_check(sc, ref, got_index):
    """the kernel's choice got_index [H, W] (Gaussian indices, -1) against the reference's T: -> three [H, W] bool maps,
    True where the rule holds or does not apply (got_index == -1):
      listed   the chosen Gaussian is an entry of the pixel's tile list
      front    the reference's T in front of it is > 0.5 (1 - MEDIAN_MARGIN)
      behind   the reference's T behind it is <= 0.5 (1 + MEDIAN_MARGIN), or it is the reference's last contributor"""
    maps = [torch.ones(sc.H, sc.W, dtype=torch.bool) for _ in range(3)]
    got_index = got_index.long()
    for tile, idx, px, py in X._tiles(sc):
        g = got_index[py, px]
        has = g >= 0
        if idx.numel() == 0:
            maps[0][py, px] = ~has
            continue
        w = ref.walk[tile]
        match = idx[None, :] == g[:, None]
        pos = match.float().argmax(dim=1)[:, None]
        listed = match.any(dim=1)
        front = w.T.gather(1, pos)[:, 0] > 0.5 * (1 - MEDIAN_MARGIN)
        behind = (w.T_behind.gather(1, pos)[:, 0] <= 0.5 * (1 + MEDIAN_MARGIN)) | (pos[:, 0] == w.j_last)
        for m, v in zip(maps, (listed, front & listed, behind & listed)):
            m[py, px] = v | ~has
    return maps


def scene_grad_median(name):
    """the first channel of the scene's grad_image"""
    return R.render_scenes()[name].grad_image[..., 0]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reference of depth scene `name`.  Computed once; do not modify."""
    base = D.reference(name)
    return reference_of(D.depth_scene(name), scene_grad_median(name), base.fragile, base.nsp)


# ---- constructed one-tile scenes: the smallest shapes at which the walk can go wrong -----------------------------------
WIDE = 4000.0   # variance in px^2: the probability stays above 0.94 over the whole 16 x 16 tile


def _one_tile_list(name, opacity, seed, narrow=(), extra_tiles=0):
    """one 16 x 16 tile (plus extra_tiles empty tiles to its right) whose list is a seeded PERMUTATION of the V wide
    Gaussians, list position k holding opacity[k]; narrow: list positions whose Gaussian is a 1 px blob at (3, 3)
    instead.  -> (depth scene with a seeded unsorted z, the Gaussian at each list position)"""
    gen = torch.Generator().manual_seed(seed)
    V = len(opacity)
    order = torch.randperm(V, generator=gen)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    uv = torch.empty(V, 2, dtype=torch.float64)
    conic = torch.empty(V, 3, dtype=torch.float64)
    opa = torch.empty(V, dtype=torch.float64)
    uv[order] = 4 + 8 * rnd(V, 2)
    conic[order] = torch.stack([WIDE * (1 + 0.2 * rnd(V)), 40 * (rnd(V) - 0.5), WIDE * (1 + 0.2 * rnd(V))], dim=1)
    opa[order] = torch.tensor(opacity, dtype=torch.float64)
    for k in narrow:
        uv[order[k]] = torch.tensor([3.0, 3.0], dtype=torch.float64)
        conic[order[k]] = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64)
    ranges = torch.tensor([0, V] + [V] * extra_tiles)
    sc = R._scene(name, 16 * (1 + extra_tiles), 16, uv, conic, opa, order, ranges, 0.0, seed + 1000)
    z = 1 + 9 * rnd(V)
    return D.as_depth_scene(sc, z.float(), sc.grad_image), order


FILLER, FAINT, STRONG = 0.003, 0.0075, 0.9   # below alpha 1/255 everywhere | a contributor of ~0.7 % | crosses 0.5 alone


def _crossing(at):
    """300 entries: 200 fillers, faint contributors (T stays above 0.6), the crossing entry at list position `at`,
    faint contributors to the end"""
    return [FILLER] * 200 + [FAINT] * (at - 200) + [STRONG] + [FAINT] * (299 - at)


@functools.lru_cache(maxsize=None)
def constructed():
    """name -> SimpleNamespace(sc, order, expect): expect is the list position every pixel of the first tile must choose
    (None: per pixel, the reference says)"""
    cases = {}

    def add(name, opacity, expect, **kw):
        sc, order = _one_tile_list(name, opacity, 900 + len(cases), **kw)
        cases[name] = SimpleNamespace(sc=sc, order=order, expect=expect)

    for at in (255, 256, 257):   # (a) either side of the forward's 256-entry chunk
        add(f"crossing_at_{at}", _crossing(at), at)
    add("first_entry_crosses", [STRONG] + [FAINT] * 20, 0)                          # (b)
    add("never_crosses", [FILLER] * 3 + [FAINT] * 40 + [FILLER] * 5, 42)            # (c) T_end ~ 0.74
    add("nobody_reaches", [STRONG, 0.5], None, narrow=(0, 1), extra_tiles=1)        # (d) a blob at (3, 3), an empty tile
    add("saturates_early", [0.4] + [0.7] * 39, 1)                                   # (e) the walk stops near entry 9
    return cases


@functools.lru_cache(maxsize=None)
def constructed_reference(name):
    """the reference of constructed()[name].  Computed once; do not modify."""
    sc = constructed()[name].sc
    base = D.reference_of(sc, sc.grad_image)
    return reference_of(sc, sc.grad_image[..., 0], base.fragile, base.nsp)
