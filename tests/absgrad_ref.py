"""References for the per-pixel absolute uv gradient (absgrad; test code only).

For pixel p and list entry k that contributes at p, in the notation of tests/render_ref64.py (_abs_sums' docstring:
W_k the walk's weight, S_k the colour behind entry k),

    dL/dalpha_k(p) = sum_ch grad_image[p, ch] (col_k[ch] W_k - S_k[ch] / (1 - alpha_k))
    g_u(p, k) = dL/dalpha_k(p) alpha_k (c dx - b dy) / det
    g_v(p, k) = dL/dalpha_k(p) alpha_k (a dy - b dx) / det
    absgrad[g] = sum over tiles, pixels, entries of (|g_u|, |g_v|)          float [V, 2], >= 0

absgrad_fp64 does not type these formulas in: per tile it hands the walk loss of render_ref64.render_fp64
((comp s + background) . grad_image, s and every decision constants) to autograd with the centres expanded to a
[pixels, entries, 2] leaf, so that the leaf's gradient IS g(p, k); it is summed with and without the sign.  The
decisions are render_fp64's: an entry is walked iff k < nsp[p], contributes iff walked and alpha >= alpha_min (the
count per pixel is asserted against the reference's), the background enters iff the final A < 0.999, s is the
reference's scale.  Not written from csrc/render.hip.

absgrad_fp32 is the same terms in float32, in the part the fp32 oracle plays for the signed gradients: it walks as
the backward does -- back to front from the fp32 forward's final weight (fw and nsp of the oracle's forward, which other
tests hold bit-equal to the kernels'), dividing by 1 - alpha at each contributor (except the one at list position
nsp - 1: the walk's scale) and adding up the colour behind -- because a forward product of (1 - alpha) measures its
own 1 - A where the weights are 1e-4 (opaque_stack: 3.0e-4 against 3e-8 to 3e-7 elsewhere), not the kernel."""
import functools

import torch

from . import render_ref64 as R
from .ref64 import sh_basis


def absgrad_fp64(sc, ref, st=R.FP32):
    """sc: a scene of render_ref64 (one coefficient), ref: render_fp64's result for it with gradients (ref.grad_image:
    zero on the fragile pixels) -> (absgrad_walk [V, 2], the signed sum of the same terms [V, 2]), float64"""
    V, W, H = sc.uv.shape[0], sc.W, sc.H
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    uv, opacity, conic = sc.uv.double(), sc.opacity.double(), sc.conic.double()
    coeff = R.scene_coeff(sc, 1).double().reshape(V, 3)
    bg = sc.bg.double()
    out_abs = torch.zeros(V, 2, dtype=torch.float64)
    out_sum = torch.zeros(V, 2, dtype=torch.float64)
    for ty in range(nty):
        for tx in range(ntx):
            tile = ty * ntx + tx
            idx = sc.sorted_g[int(sc.ranges[tile]):int(sc.ranges[tile + 1])].long()
            px, py = R._tile_pixels(tx, ty, W, H)
            P, L = px.numel(), idx.numel()
            if L == 0:
                continue
            centre = uv[idx][None, :, :].expand(P, L, 2).clone().requires_grad_(True)   # one centre per (pixel, entry)
            dx = px.double()[:, None] - centre[:, :, 0]
            dy = py.double()[:, None] - centre[:, :, 1]
            a = (conic[idx, 0] + st.blur)[None, :]
            b = (conic[idx, 1] / 2)[None, :]
            c = (conic[idx, 2] + st.blur)[None, :]
            m = (c * dx * dx - 2 * b * dx * dy + a * dy * dy) / (a * c - b * b)
            alpha = torch.where(m > 0, opacity[idx, 0][None, :] * torch.exp(-m / 2), torch.zeros_like(m))
            with torch.no_grad():
                walked = torch.arange(L)[None, :] < ref.nsp[py, px].long()[:, None]
                contrib = walked & (alpha >= st.alpha_min)
                assert torch.equal(contrib.sum(dim=1).int(), ref.contrib[py, px])
            one_minus = 1 - alpha * contrib
            T = torch.cat([torch.ones(P, 1, dtype=torch.float64), torch.cumprod(one_minus, dim=1)[:, :-1]], dim=1)
            T_fin = one_minus.prod(dim=1)
            with torch.no_grad():
                with_bg = (1 - T_fin) < R.BG_BELOW
            col = sh_basis(torch.zeros(P, 3, dtype=torch.float64), 1)[:, None, :] * coeff[idx][None, :, :]   # Y_0 coeff
            comp = ((alpha * T * contrib)[:, :, None] * col).sum(dim=1)
            back = bg[None, :] * (T_fin * with_bg)[:, None]
            loss = ((comp * ref.scale[py, px][:, None] + back) * ref.grad_image[py, px]).sum()
            g, = torch.autograd.grad(loss, centre)
            out_abs.index_add_(0, idx, g.abs().sum(dim=0))
            out_sum.index_add_(0, idx, g.sum(dim=0))
    return out_abs, out_sum


def absgrad_fp32(sc, fw, nsp, grad_image, st=R.FP32):
    """the same terms in float32 on the backward's walk (module docstring); fw [H, W] float32 and nsp [H, W] int32 of
    the fp32 forward, grad_image [H, W, 3] -> absgrad [V, 2] (sums in float64 of float32 terms: the kernel's own
    summation noise is what the measure is to see, not this one's)"""
    f32 = torch.float32
    V, W, H = sc.uv.shape[0], sc.W, sc.H
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    uv, opacity, conic = sc.uv.to(f32), sc.opacity.to(f32), sc.conic.to(f32)
    Y0 = sh_basis(torch.zeros(1, 3, dtype=torch.float64), 1)[0, 0].to(f32)
    coeff = R.scene_coeff(sc, 1).to(f32).reshape(V, 3) * Y0
    bg = sc.bg.to(f32)
    gi_all = grad_image.to(f32)
    out = torch.zeros(V, 2, dtype=torch.float64)
    blur = torch.tensor(st.blur, dtype=f32)
    for ty in range(nty):
        for tx in range(ntx):
            tile = ty * ntx + tx
            idx = sc.sorted_g[int(sc.ranges[tile]):int(sc.ranges[tile + 1])].long()
            px, py = R._tile_pixels(tx, ty, W, H)
            n = nsp[py, px].long()
            L = min(idx.numel(), int(n.max())) if idx.numel() else 0
            if L == 0:
                continue
            idx = idx[:L]
            P = px.numel()
            dx = px.to(f32)[:, None] - uv[idx, 0][None, :]
            dy = py.to(f32)[:, None] - uv[idx, 1][None, :]
            a = (conic[idx, 0] + blur)[None, :]
            b = (conic[idx, 1] / 2)[None, :]
            c = (conic[idx, 2] + blur)[None, :]
            det = a * c - b * b
            m = (c * dx * dx - 2 * b * dx * dy + a * dy * dy) / det
            alpha = torch.where(m > 0, opacity[idx, 0][None, :] * torch.exp(-m / 2), torch.zeros_like(m))
            pos = torch.arange(L)[None, :]
            contrib = (pos < n[:, None]) & (alpha >= st.alpha_min)
            divides = contrib & (pos < (n - 1)[:, None])
            oma = 1 - alpha
            gi = gi_all[py, px]
            col = coeff[idx]                                   # [L, 3]
            weight = fw[py, px].to(f32).clone()
            behind = torch.zeros(P, 3, dtype=f32)
            started = torch.zeros(P, dtype=torch.bool)
            ga = torch.zeros(P, L, dtype=f32)
            for k in range(L - 1, -1, -1):
                ck = contrib[:, k]
                if not bool(ck.any()):
                    continue
                first = ck & ~started                          # the background behind the pixel's last contributor
                bw = weight - alpha[:, k] * weight
                behind = torch.where((first & (bw > 0.001))[:, None], behind + bg[None, :] * bw[:, None], behind)
                started = started | ck
                weight = torch.where(divides[:, k], weight / oma[:, k], weight)
                gk = ((col[k][None, :] * weight[:, None] - behind / oma[:, k][:, None]) * gi).sum(dim=1)
                ga[:, k] = torch.where(ck, gk, torch.zeros_like(gk))
                behind = torch.where(ck[:, None], behind + col[k][None, :] * (alpha[:, k] * weight)[:, None], behind)
            f = ga * alpha / det
            e = torch.stack([(f * (c * dx - b * dy)).abs(), (f * (a * dy - b * dx)).abs()], dim=2)   # [P, L, 2] float32
            out.index_add_(0, idx, e.double().sum(dim=0))
    return out


def noise_measure(got, ref, abs_sum):
    """max |got - ref| / abs_sum over the elements somebody contributes to (tests/test_gpu_render_ref64.py's)"""
    a = abs_sum.double().reshape(-1)
    d = (got.double().reshape(-1) - ref.double().reshape(-1)).abs()
    return float((d[a > 0] / a[a > 0]).max()) if bool((a > 0).any()) else 0.0


@functools.lru_cache(maxsize=None)
def scene_absgrad(name):
    """per scene of render_scenes(), one coefficient, computed once (do not modify): SimpleNamespace-like dict with
    ref (render_fp64, FP32 settings), orc (the fp32 oracle, exact mode, on ref.grad_image), absgrad / signed (fp64),
    restated (fp32 walk), measure_restated and measure_oracle (the oracle's signed g_uv), both over abs_walk g_uv"""
    from .test_render_ref64 import oracle_run
    sc = R.render_scenes()[name]
    ref = R.reference(name, 1, "fp32")
    orc = oracle_run(sc, 1, torch.float32, ref.grad_image, exact=True)
    return evaluate(sc, ref, orc)


def evaluate(sc, ref, orc):
    absgrad, signed = absgrad_fp64(sc, ref)
    restated = absgrad_fp32(sc, orc["fw"], orc["nsp"], ref.grad_image)
    den = ref.abs_walk["g_uv"]
    return dict(sc=sc, ref=ref, orc=orc, absgrad=absgrad, signed=signed, restated=restated,
                measure_restated=noise_measure(restated, absgrad, den),
                measure_oracle=noise_measure(orc["g_uv"], ref.grad_walk["g_uv"], den))
