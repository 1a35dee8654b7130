"""A plain float64 reference of the render stage (compositing forward and its derivative) and the small scenes the
render kernels are held to it on (test code only).

render_fp64 is written from the formulas with torch autograd, not from csrc/render.hip or oracle/gs_oracle.cpp.  Per
tile it forms [pixels, list entries] tensors.  For pixel (px, py) and list entry g, in list order:

  d      = (px - u_g, py - v_g)
  a, b, c = conic0 + blur, conic1 / 2, conic2 + blur
  m      = (c dx^2 - 2 b dx dy + a dy^2) / (a c - b^2)
  alpha  = opacity exp(-m / 2) if m > 0 else 0        (a Gaussian centred exactly on a pixel contributes nothing)
  the entry contributes iff alpha >= alpha_min
  the walk stops before the first entry at which the accumulated opacity A exceeds 0.9999
  weight = alpha (1 - A),  A += weight
  colour = sum_s Y_s(ray of the pixel) coeff_s        (one coefficient: Y_0 coeff_0, ref64.sh_basis's fp32 constants)
  image  = sum weight colour + background (1 - A) if the final A < 0.999

  FP64: blur = 0,    alpha_min = 0               (the float64 kernels: every walked entry contributes)
  FP32: blur = 0.25, alpha_min = 0.00392156862   (the float32 kernels)

The decisions (contributes / stops / background) are taken under no_grad and are constants of the derivative.
num_splats counts the entries walked, contributing or not; the final weight is 1 - A before the last contributing entry.

Two sets of gradients come back for a grad_image.  `grad` is the true derivative of the image above.  `grad_walk` is
what the reference's backward walk returns (render_backward.cu:167-233 read as formulas, SURVEY.md section 6's probe):
it starts from the final weight T_j of the last contributing entry j and divides it by (1 - alpha_k) at every
contributing entry except the one at list position num_splats - 1.  Where the last walked entry contributes -- every
pixel of the float64 kernels, every pixel that stopped because it saturated -- the two are the same thing.  Where
skipped entries trail the last contributor (float32 only) the walk divides at j too, and every weight of the pixel
comes out scaled by s = 1 / (1 - alpha_j): the compositing part of the pixel's gradient is s times the true one, the
background part (formed from T_j before the division) is not scaled.  The kernels' `exact` backward mode keeps this
(it only replaces render_backward.cu:185's chunk-local index by the global one), so float32 kernels are compared with
`grad_walk`, and the share of pixels with s != 1 is reported next to it.  s is a constant of the derivative.

`abs` / `abs_walk`: per gradient element the float64 sum over pixels of the magnitudes of the leaf terms of its
formula (every product that enters a sum or a difference), the scale of an fp32 evaluation's unavoidable noise.

fragile [H, W]: a decision of the pixel sits within relative margin MARGIN of its threshold -- some walked alpha
within MARGIN alpha_min of alpha_min, some prefix A within MARGIN 0.9999 of 0.9999, the final A within MARGIN 0.999 of
0.999, some m != 0 with |m| <= MARGIN.  (m == 0 exactly needs dx == dy == 0, which every precision sees alike: the
inputs are fp32 values.)  A scene's grad_image is zero on its fragile pixels, so a flipped decision there cannot move
any gradient.  The reference raises if a contributing alpha exceeds 0.99: the reference's backward caps alpha at 0.9999
where its forward does not, and the scenes stay clear of that."""
import functools
from types import SimpleNamespace

import torch

from .ref64 import sh_basis

FP64 = SimpleNamespace(name="fp64", blur=0.0, alpha_min=0.0, dtype=torch.float64)
FP32 = SimpleNamespace(name="fp32", blur=0.25, alpha_min=0.00392156862, dtype=torch.float32)
SAT = 0.9999       # the walk stops once A exceeds it
BG_BELOW = 0.999   # the background is added below it
ALPHA_MAX = 0.99
# The margin of `fragile`.  CHOSEN from the number format, not measured: the measurement found nothing to measure.
# On the CPU the fp32 oracle (oracle/gs_oracle.cpp, deterministic exponential) and
# this reference with the FP32 settings take the same decisions on EVERY pixel of render_scenes() with 1, 4, 9 and 16
# coefficients -- no pixel flips, so the scenes themselves ask for no margin at all
# (tests/test_render_ref64.py::test_margin_is_no_smaller_than_the_scenes_need keeps that measured).  The constant is
# therefore what the number format asks for: an fp32 A near 0.9999 carries a few ulp (6e-8 each) of accumulated
# rounding, 2^-21 = 4.8e-7 is 8 of them.  A wider margin costs pixels: a pixel that crosses 0.9999 in a step
# alpha (1 - A) ~ 1e-4 alpha is fragile with probability ~ 2 MARGIN / (1e-4 alpha), 1 % at alpha = 0.5.
MARGIN = 2.0 ** -21
GRAD_KEYS = ("g_rgb", "g_opacity", "g_uv", "g_conic")


def _tile_pixels(tx, ty, W, H):
    xs = torch.arange(tx * 16, min(tx * 16 + 16, W))
    ys = torch.arange(ty * 16, min(ty * 16 + 16, H))
    py, px = torch.meshgrid(ys, xs, indexing="ij")
    return px.reshape(-1), py.reshape(-1)


def closeness(alpha, walked, A_prefix, A_final, m, st):
    """per pixel the smallest relative distance of a decision from its threshold (inf where there is none)"""
    inf = torch.full_like(alpha, float("inf"))
    c = torch.where(walked & (m != 0), m.abs(), inf).amin(dim=1)
    if st.alpha_min > 0:
        c = torch.minimum(c, torch.where(walked, (alpha - st.alpha_min).abs() / st.alpha_min, inf).amin(dim=1))
    c = torch.minimum(c, ((A_prefix - SAT).abs() / SAT).amin(dim=1))
    return torch.minimum(c, (A_final - BG_BELOW).abs() / BG_BELOW)


def render_fp64(uv, opacity, coeff, conic, rays, ranges, sorted_g, bg, W, H, st, grad_image=None, margin=MARGIN):
    """uv [V,2], opacity [V,1], coeff [V,3] or [V,3,n_sh], conic [V,3], rays [H,W,3] unit (unused with one coefficient),
    ranges [tiles+1], sorted_g [S], bg [3]; st = FP64 or FP32.  Everything is taken to float64 first.
    -> SimpleNamespace(image, nsp, contrib (count per pixel), fw, fragile, closeness, scale (s of the module docstring)
    and, with grad_image, grad / grad_walk / abs / abs_walk (dicts over GRAD_KEYS, shaped like the inputs) and
    used [V] (contributes at a pixel whose grad_image is non-zero))."""
    leaf = lambda x: x.detach().double().clone().requires_grad_(grad_image is not None)
    uv, opacity, conic = leaf(uv), leaf(opacity), leaf(conic)
    coeff_in = leaf(coeff)
    V = uv.shape[0]
    cf = coeff_in.reshape(V, 3, -1)
    n_sh = cf.shape[2]
    bg = bg.detach().double()
    ntx = (W + 15) // 16
    nty = (H + 15) // 16
    image = torch.zeros(H, W, 3, dtype=torch.float64)
    nsp = torch.zeros(H, W, dtype=torch.int32)
    ncontrib = torch.zeros(H, W, dtype=torch.int32)
    fw = torch.zeros(H, W, dtype=torch.float64)
    close = torch.full((H, W), float("inf"), dtype=torch.float64)
    scale = torch.ones(H, W, dtype=torch.float64)
    used = torch.zeros(V, dtype=torch.bool)
    gi_all = None if grad_image is None else grad_image.detach().double()
    loss = torch.zeros((), dtype=torch.float64)
    loss_walk = torch.zeros((), dtype=torch.float64)
    ab = {s: dict(g_rgb=torch.zeros(V, 3, n_sh, dtype=torch.float64), g_opacity=torch.zeros(V, 1, dtype=torch.float64),
                  g_uv=torch.zeros(V, 2, dtype=torch.float64), g_conic=torch.zeros(V, 3, dtype=torch.float64))
          for s in ("abs", "abs_walk")}
    for ty in range(nty):
        for tx in range(ntx):
            tile = ty * ntx + tx
            idx = sorted_g[int(ranges[tile]):int(ranges[tile + 1])].long()
            px, py = _tile_pixels(tx, ty, W, H)
            P, L = px.numel(), idx.numel()
            if L == 0:
                image[py, px] = bg   # A = 0 < 0.999
                close[py, px] = abs(0.0 - BG_BELOW) / BG_BELOW
                continue
            dx = px.double()[:, None] - uv[idx, 0][None, :]
            dy = py.double()[:, None] - uv[idx, 1][None, :]
            a = (conic[idx, 0] + st.blur)[None, :]
            b = (conic[idx, 1] / 2)[None, :]
            c = (conic[idx, 2] + st.blur)[None, :]
            det = a * c - b * b
            q = c * dx * dx - 2 * b * dx * dy + a * dy * dy
            m = q / det
            prob = torch.exp(-m / 2)
            opa = opacity[idx, 0][None, :]
            alpha = torch.where(m > 0, opa * prob, torch.zeros_like(m))
            with torch.no_grad():
                cand = alpha >= st.alpha_min
            # T[:, k] = 1 - A before entry k (as if nobody stopped: a stopped pixel ignores what comes after)
            one_minus = 1 - alpha * cand
            T_incl = torch.cumprod(one_minus, dim=1)
            T = torch.cat([torch.ones(P, 1, dtype=torch.float64), T_incl[:, :-1]], dim=1)
            with torch.no_grad():
                walked = (1 - T) <= SAT                   # A is monotone: the walk is a prefix of the list
                contrib = cand & walked
            T_fin = torch.where(contrib, one_minus, torch.ones_like(one_minus)).prod(dim=1)   # 1 - final A
            with torch.no_grad():
                if bool((contrib & (alpha > ALPHA_MAX)).any()):
                    raise ValueError("a contributing alpha exceeds 0.99: outside what the reference models")
                n_walk = walked.sum(dim=1)
                any_c = contrib.any(dim=1)
                pos = torch.arange(L)[None, :]
                j_last = torch.where(contrib, pos, torch.full_like(pos, -1)).amax(dim=1)   # -1: none
                A_final = 1 - T_fin.detach()
                with_bg = A_final < BG_BELOW
                jc = j_last.clamp(min=0)[:, None]
                T_last = torch.where(any_c, T.gather(1, jc)[:, 0], torch.zeros(P, dtype=torch.float64))
                # the walk's scale: the last walked entry is a skipped one behind the last contributor
                a_last = alpha.gather(1, jc)[:, 0]
                s = torch.where(any_c & (j_last < n_walk - 1), 1 / (1 - a_last), torch.ones_like(a_last))
                A_prefix = torch.where(walked, 1 - T, torch.zeros_like(T))
                A_prefix = torch.cat([A_prefix, A_final[:, None]], dim=1)
                cl = closeness(alpha, walked, A_prefix, A_final, m, st)
            if n_sh > 1:
                Y = sh_basis(rays[py, px].double(), n_sh)          # [P, n_sh]
            else:
                Y = sh_basis(torch.zeros(P, 3, dtype=torch.float64), 1)
            col = torch.einsum("ps,lcs->plc", Y, cf[idx])          # [P, L, 3]
            wgt = alpha * T * contrib
            comp = (wgt[:, :, None] * col).sum(dim=1)              # [P, 3]
            back = bg[None, :] * (T_fin * with_bg)[:, None]
            image[py, px] = (comp + back).detach()
            nsp[py, px] = n_walk.int()
            ncontrib[py, px] = contrib.sum(dim=1).int()
            fw[py, px] = T_last
            close[py, px] = cl
            scale[py, px] = s
            if gi_all is None:
                continue
            gi = gi_all[py, px]
            gi = gi * (cl > margin)[:, None]
            loss = loss + ((comp + back) * gi).sum()
            loss_walk = loss_walk + ((comp * s[:, None] + back) * gi).sum()
            with torch.no_grad():
                live = contrib & (gi.abs().sum(dim=1) > 0)[:, None]
                used[idx[live.any(dim=0)]] = True
                _abs_sums(ab["abs"], idx, torch.ones_like(s), gi, Y, col, alpha, prob, opa, T, contrib, T_fin * with_bg,
                          bg, dx, dy, a, b, c, det)
                _abs_sums(ab["abs_walk"], idx, s, gi, Y, col, alpha, prob, opa, T, contrib, T_fin * with_bg, bg, dx, dy,
                          a, b, c, det)
    out = SimpleNamespace(image=image, nsp=nsp, contrib=ncontrib, fw=fw, closeness=close, fragile=close <= margin,
                          scale=scale, n_sh=n_sh)
    if gi_all is not None:
        leaves = (coeff_in, opacity, uv, conic)
        for name, l in (("grad", loss), ("grad_walk", loss_walk)):
            if l.requires_grad:
                g = torch.autograd.grad(l, leaves, retain_graph=True, allow_unused=True)
            else:
                g = (None,) * 4
            setattr(out, name, {k: (torch.zeros_like(x) if gr is None else gr.detach())
                                for k, x, gr in zip(GRAD_KEYS, leaves, g)})
        for s in ("abs", "abs_walk"):
            ab[s]["g_rgb"] = ab[s]["g_rgb"].reshape(coeff_in.shape)
            setattr(out, s, ab[s])
        out.used = used
    return out


def _abs_sums(acc, idx, s, gi, Y, col, alpha, prob, opa, T, contrib, T_bg, bg, dx, dy, a, b, c, det):
    """adds one tile's leaf magnitudes: with W_k = s T_k the walk's weight, S_k = bg T_bg + s sum_{j>k} col_j alpha_j T_j
    the colour behind entry k,
      d image / d coeff_{k,ch,s} = Y_s alpha_k W_k                             (one leaf)
      d image_ch / d alpha_k     = col_k W_k - S_k / (1 - alpha_k)             (two leaves)
      d alpha / d opacity = prob,  d alpha / d m = -alpha / 2,  and with q = c dx^2 - 2 b dx dy + a dy^2 (three leaves)
      dm/du = -(2 c dx - 2 b dy) / det,  dm/dv = -(2 a dy - 2 b dx) / det,
      dm/d conic0 = dy^2 / det - c q / det^2,  dm/d conic1 = -dx dy / det + b q / det^2,
      dm/d conic2 = dx^2 / det - a q / det^2"""
    Wk = s[:, None] * T * contrib
    term = (alpha * Wk)[:, :, None] * col                               # [P, L, 3] what entry k adds to the image
    behind = term.sum(dim=1, keepdim=True) - torch.cumsum(term, dim=1) + (bg[None, :] * T_bg[:, None])[:, None, :]
    agi = gi.abs()[:, None, :]
    ga = (((col * Wk[:, :, None]).abs() + (behind / (1 - alpha)[:, :, None]).abs()) * agi).sum(dim=2) * contrib
    acc["g_rgb"].index_add_(0, idx, torch.einsum("pl,pc,ps->lcs", alpha * Wk, gi.abs(), Y.abs()))
    acc["g_opacity"].index_add_(0, idx, (prob * ga).sum(dim=0)[:, None])
    gm = 0.5 * prob * opa.abs() * ga
    rd = 1 / det
    qa = (a.abs() * dy * dy + 2 * (b * dx * dy).abs() + c.abs() * dx * dx) * rd * rd
    acc["g_uv"].index_add_(0, idx, torch.stack([((2 * (c * dx).abs() + 2 * (b * dy).abs()) * rd * gm).sum(dim=0),
                                                ((2 * (a * dy).abs() + 2 * (b * dx).abs()) * rd * gm).sum(dim=0)], dim=1))
    acc["g_conic"].index_add_(0, idx, torch.stack([((dy * dy * rd + c.abs() * qa) * gm).sum(dim=0),
                                                   (((dx * dy).abs() * rd + b.abs() * qa) * gm).sum(dim=0),
                                                   ((dx * dx * rd + a.abs() * qa) * gm).sum(dim=0)], dim=1))


# ---- scenes ---------------------------------------------------------------------------------------------------------
def _oracle_lists(uv, conic, depth, W, H, mh=3.0):
    from oracle import gs_oracle
    xyz_c = torch.cat([torch.zeros(uv.shape[0], 2), depth[:, None]], dim=1).float().contiguous()
    return gs_oracle.get_sorted_gaussian_list(1024, uv.float().contiguous(), xyz_c, conic.float().contiguous(),
                                              (W + 15) // 16, (H + 15) // 16, mh)


def _scene(name, W, H, uv, conic, opacity, sorted_g, ranges, bg, seed, exact_only=False):
    gen = torch.Generator().manual_seed(seed)
    V = uv.shape[0]
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    coeff = torch.cat((rnd(V, 3, 1) / 0.28209479177387814, 0.3 * (rnd(V, 3, 15) - 0.5)), dim=2)
    rays = torch.randn(H, W, 3, generator=gen, dtype=torch.float64)
    rays = rays / rays.norm(dim=2, keepdim=True)
    gi = torch.randn(H, W, 3, generator=gen, dtype=torch.float64)
    f = lambda x: x.float().contiguous()   # the inputs are fp32 values in every precision
    return SimpleNamespace(name=name, W=W, H=H, V=V, uv=f(uv), conic=f(conic), opacity=f(opacity).reshape(V, 1),
                           coeff16=f(coeff), rays=f(rays), grad_image=f(gi), bg=torch.full((3,), float(bg)),
                           sorted_g=sorted_g.int().contiguous(), ranges=ranges.int().contiguous(),
                           exact_only=exact_only)


def scene_coeff(sc, n_sh):
    """the scene's colour input with n_sh coefficients: [V, 3] for one, [V, 3, n_sh] otherwise"""
    return sc.coeff16[:, :, 0].contiguous() if n_sh == 1 else sc.coeff16[:, :, :n_sh].contiguous()


def _random_frame(name, W, H, N, seed, bg, lone=None):
    """N Gaussians over the top left of a W x H frame (tiles at the right and bottom edges stay empty or nearly so),
    lists from the oracle's tile culling; lone = (u, v): one small Gaussian alone in its tile"""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    uv = torch.stack([0.4 * W * rnd(N), 0.6 * H * rnd(N)], dim=1)
    sig = 1.0 + 2.5 * rnd(N, 2)
    rho = 1.6 * (rnd(N) - 0.5)
    conic = torch.stack([sig[:, 0] ** 2, 2 * rho * sig[:, 0] * sig[:, 1], sig[:, 1] ** 2], dim=1)
    opacity = 0.05 + 0.9 * rnd(N)
    if lone is not None:
        uv = torch.cat([uv, torch.tensor([lone], dtype=torch.float64)])
        conic = torch.cat([conic, torch.tensor([[0.8, 0.1, 0.6]], dtype=torch.float64)])
        opacity = torch.cat([opacity, torch.tensor([0.7], dtype=torch.float64)])
    depth = 1 + 9 * rnd(uv.shape[0])
    sorted_g, ranges = _oracle_lists(uv, conic, depth, W, H)
    return _scene(name, W, H, uv, conic, opacity, sorted_g, ranges, bg, seed + 1000)


def _one_tile(name, V, seed, bg, opacity, conic_lo=20.0, conic_hi=50.0, exact_only=False):
    """one 16 x 16 tile whose list holds all V splats in index order (hand-made list)"""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    uv = rnd(V, 2) * 16
    conic = torch.stack([conic_lo + (conic_hi - conic_lo) * rnd(V), 4 * (rnd(V) - 0.5),
                         conic_lo + (conic_hi - conic_lo) * rnd(V)], dim=1)
    return _scene(name, 16, 16, uv, conic, opacity(rnd, V), torch.arange(V), torch.tensor([0, V]), bg, seed + 1000,
                  exact_only)


def _edge_cases(seed, bg):
    """32 x 16, two tiles: Gaussians whose centre is a pixel (m = 0 there), a needle, and Gaussians on the border
    between the tiles (the oracle's lists name them in both)"""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    uv = torch.tensor([[5.0, 7.0], [20.0, 3.0], [16.0, 8.0], [15.4, 4.3], [9.3, 11.6], [24.7, 9.2], [15.9, 12.1],
                       [3.2, 2.9]], dtype=torch.float64)
    conic = torch.tensor([[9.0, 2.0, 6.0], [4.0, -1.0, 5.0], [12.0, 3.0, 7.0], [16.0, 0.5, 9.0],
                          [60.0, 2 * 0.995 * (60.0 * 0.4) ** 0.5, 0.4],      # the needle: correlation 0.995
                          [7.0, -3.0, 8.0], [25.0, 6.0, 20.0], [2.0, 0.3, 3.0]], dtype=torch.float64)
    opacity = 0.15 + 0.75 * rnd(uv.shape[0])
    depth = 1 + 9 * rnd(uv.shape[0])
    sorted_g, ranges = _oracle_lists(uv, conic, depth, 32, 16)
    return _scene("edge_cases_32x16", 32, 16, uv, conic, opacity, sorted_g, ranges, bg, seed + 1000)


@functools.lru_cache(maxsize=None)
def render_scenes():
    """name -> scene (see the module docstring of tests/test_render_ref64.py for what each one is aimed at)"""
    scenes = [
        _random_frame("partial_48x40", 48, 40, 40, 11, 0.5, lone=(44.3, 36.2)),
        _random_frame("partial_33x17", 33, 17, 24, 12, 0.0, lone=(32.2, 16.4)),
        _random_frame("strip_70x13", 70, 13, 36, 13, 0.5, lone=(67.6, 5.3)),
        _random_frame("partial_48x40_black", 48, 40, 40, 14, 0.0),
        _one_tile("faint_300", 300, 21, 0.5, lambda rnd, V: 0.002 + 0.018 * rnd(V)),
        _one_tile("opaque_stack", 70, 22, 0.0, lambda rnd, V: 0.35 + 0.63 * rnd(V), conic_lo=60.0, conic_hi=800.0),
        _one_tile("long_1100", 1100, 23, 0.5, lambda rnd, V: 0.003 + 0.009 * rnd(V), exact_only=True),
        _edge_cases(24, 0.5),
    ]
    return {s.name: s for s in scenes}


def max_list(sc):
    return int((sc.ranges[1:] - sc.ranges[:-1]).max())


def first_chunk(sc, st, n_sh):
    """the scene's lists fit the reference backward's first chunk (render_backward.cu:402-568), where its chunk-local
    index is the global one and compat mode is exact mode"""
    table = {"fp32": {1: 960, 4: 576, 9: 320, 16: 160}, "fp64": {1: 320, 4: 160, 9: 128, 16: 64}}
    return max_list(sc) <= table[st.name][n_sh]


@functools.lru_cache(maxsize=None)
def reference(name, n_sh, st_name, unscaled_only=False):
    """render_fp64 of scene `name` with n_sh coefficients under the FP64 / FP32 settings, with gradients for the
    scene's grad_image (zeroed on the fragile pixels, also returned as .grad_image).  unscaled_only: grad_image is
    zero on the pixels whose walk gradient is scaled (scale != 1) too, so `grad_walk` IS the true derivative `grad`.
    Computed once; do not modify."""
    sc = render_scenes()[name]
    st = FP64 if st_name == "fp64" else FP32
    gi = sc.grad_image
    if unscaled_only:
        gi = gi * (reference(name, n_sh, st_name).scale == 1)[:, :, None]
    ref = render_fp64(sc.uv, sc.opacity, scene_coeff(sc, n_sh), sc.conic, sc.rays, sc.ranges, sc.sorted_g, sc.bg,
                      sc.W, sc.H, st, gi)
    ref.grad_image = (gi.double() * (~ref.fragile)[:, :, None]).contiguous()
    return ref


def run_module(mod, dev, sc, n_sh, dtype, grad_image):
    """the scene through a provider of the reference's render_tiles_cuda / render_tiles_backward_cuda (the oracle on
    the CPU, a HIP backend on the GPU) -> dict image, nsp, fw, g_rgb, g_opacity, g_uv, g_conic on the CPU"""
    c = lambda x: x.to(dev).to(dtype).contiguous() if x.is_floating_point() else x.to(dev).contiguous()
    H, W = sc.H, sc.W
    img = torch.zeros(H, W, 3, dtype=dtype, device=dev)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=dev)
    fw = torch.zeros(H, W, dtype=dtype, device=dev)
    rays = sc.rays if n_sh > 1 else torch.zeros(1, 1, 1)
    args = (c(sc.uv), c(sc.opacity), c(scene_coeff(sc, n_sh)), c(sc.conic), c(rays), c(sc.ranges), c(sc.sorted_g),
            c(sc.bg))
    mod.render_tiles_cuda(*args, nsp, fw, img)
    grads = [torch.zeros_like(x) for x in (args[2], args[1], args[0], args[3])]
    mod.render_tiles_backward_cuda(*args, nsp, fw, c(grad_image), *grads)
    out = dict(image=img.cpu(), nsp=nsp.cpu(), fw=fw.cpu())
    out.update({k: g.cpu() for k, g in zip(GRAD_KEYS, grads)})
    return out
