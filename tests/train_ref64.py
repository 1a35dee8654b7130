"""float64 references and noise-aware measures for the training-step kernels behind the rasterizer: k_adam
(csrc/train_ops.hip + csrc/adam_math.h), k_ssim_l1 / k_loss_finish (csrc/loss.hip).  TEST INFRASTRUCTURE ONLY.
tests/test_train_ref64.py holds these references to PyTorch's own float64 results on the CPU and shows that correct
fp32 implementations meet the bounds; tests/test_gpu_train_ref64.py holds the kernels to them.

Adam.  One step in float64 of adam_math.h's four lines on the fp32 inputs, with the scalars rounded to fp32 where
adam_shared / adam_scalars round them.  Stage-wise: p' is formed from the m' and v' that the implementation under test
produced (fp32), so no error is carried from one stage or one step into the next.  Bound per element

    |got - ref| <= (K + 1) 2^-24 abs_sum + 2^-126

abs_sum: the sum of the magnitudes of the terms of the expression.  K: the number of fp32 roundings in the expression
as written (the library is built with -ffp-contract=off: no rounding is fused away; an FMA in another correct
implementation only removes one).  With u = 2^-24 and every rounding a factor (1 + d), |d| <= u:

    m' = m + w1 (g - m)               fl(g - m), fl(w1 .), fl(m + .): the term t = w1 (g - m) carries 2 u |t|, the
                                      sum u (|m| + |t|)                                              K = 3
    v' = v beta2 + (w2 g) g           fl(v beta2), fl(w2 g), fl(. g), fl(+)                           K = 4
    p' = p + (neg_step m') / denom    denom = sqrt(v') / bc2_sqrt + eps: sqrt, divide, add of two non-negative
                                      terms (relative error of the sum <= the larger of its terms'), then the
                                      multiply, the divide and the add to p                           K = 6

One more u for the second-order terms (the products of the d's; (1 + u)^6 - 1 < 7 u).  fp32 divide and sqrt are
correctly rounded in this build: hipcc's default is -fhip-fp32-correctly-rounded-divide-sqrt, csrc/Makefile passes
neither -fno-hip-fp32-correctly-rounded-divide-sqrt nor -ffast-math / -cl-fp32-correctly-rounded-divide-sqrt
overrides, and adam_math.h uses `/` and __builtin_sqrtf (no __fdividef, no rcp/rsq intrinsics): no ulp excess is
added to K.  2^-126 (the smallest normal) makes the bound indifferent to whether a denormal intermediate is kept
(error <= 2^-150) or flushed (error < 2^-126); the regimes of the tests keep neg_step m' normal, so no flushed
product is magnified by a small denom.

Loss.  The reference is oracle/loss_oracle.py evaluated in float64 (pinned to closed forms by
tests/test_ssim_known_answers.py).  Two fp32 restatements supply the scale of the unavoidable fp32 error:
    ssim_map_2d    loss_oracle's own lines (reflect padding, one 121-tap grouped conv2d, double crop), returning the map
    ssim_map_sep   the same formula over the valid windows only, an 11-tap row pass and then an 11-tap column pass
                   accumulated tap by tap (the kernel's summation order)
The variances are E[x^2] - mu^2 next to c2 = 9e-4: in a bright flat region fp32 loses most of their digits, so the
error of a correct fp32 evaluation depends on the image and a fixed tolerance is either too tight
there or blind elsewhere.  Two correct summation orders differ per pixel by far more than either's error AT that
pixel where one happens to be exact, so the envelope of a pixel is the largest |fp32 2-D restatement - reference| over
the 21x21 neighbourhood and the channels: all pixels that share a window with it."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss_oracle

U = 2.0 ** -24
TINY = 2.0 ** -126
R_MAX = 8.0   # tests/test_gpu_general_cameras.py


def f32(x):
    """the double that equals x rounded to fp32"""
    return float(np.float32(x))


# ---- Adam ------------------------------------------------------------------------------------------------------------
ADAM_K = {"m": 3 + 1, "v": 4 + 1, "p": 6 + 1}   # roundings + 1 (module docstring)
# config.py of the reference: base_lr 0.002 times the per-group multipliers (tests/test_gpu_train_ops.py)
LRS = (0.002 * 0.1, 0.002 * 2, 0.002 * 5, 0.002 * 10, 0.002 * 2, 0.002 * 0.1)


def adam_scalars(lr, step, beta1, beta2, eps):
    """the six fp32 scalars of one tensor's step (adam_math.h: adam_shared, adam_scalars), as doubles.
    step: the 1-based count after the increment"""
    bc1 = 1.0 - math.pow(beta1, float(step))
    bc2 = 1.0 - math.pow(beta2, float(step))
    return dict(w1=f32(1.0 - beta1), beta2=f32(beta2), w2=f32(1.0 - beta2), eps=f32(eps),
                neg_step=f32(-(lr / bc1)), bc2_sqrt=f32(math.sqrt(bc2)))


def adam_moments(g, m, v, sc):
    """-> (m', |.| sum), (v', |.| sum) in float64"""
    g, m, v = g.double(), m.double(), v.double()
    t = sc["w1"] * (g - m)
    a, b = v * sc["beta2"], sc["w2"] * g * g
    return (m + t, m.abs() + t.abs()), (a + b, a.abs() + b.abs())


def adam_param(p, m_new, v_new, sc):
    """-> (p', |.| sum) in float64 from the new moments"""
    p, m_new, v_new = p.double(), m_new.double(), v_new.double()
    upd = sc["neg_step"] * m_new / (v_new.sqrt() / sc["bc2_sqrt"] + sc["eps"])
    return p + upd, p.abs() + upd.abs()


def _score(got, ref, abs_sum, ok):
    """max over the elements `ok` of (|got - ref| - 2^-126)+ / (2^-24 abs_sum)"""
    if not bool(ok.any()):
        return 0.0
    d = ((got.double() - ref).abs() - TINY).clamp(min=0)[ok]
    a = abs_sum[ok] * U
    r = torch.where(d == 0, torch.zeros_like(d), d / a)
    return float(r.max())


def adam_scores(before, after, lr, step, beta1, beta2, eps):
    """before = (p, g, m, v), after = (p', m', v') of one step of the implementation under test (fp32 CPU tensors, any
    shape).  -> {"m", "v", "p"}: the largest error in units of 2^-24 abs_sum (after the 2^-126 allowance) over the
    elements whose reference value is finite, and "nonfinite": the boolean masks of the non-finite elements of
    (p', m', v') of the implementation"""
    p, g, m, v = (x.detach().reshape(-1) for x in before)
    p1, m1, v1 = (x.detach().reshape(-1) for x in after)
    sc = adam_scalars(lr, step, beta1, beta2, eps)
    (m_ref, m_abs), (v_ref, v_abs) = adam_moments(g, m, v, sc)
    p_ref, p_abs = adam_param(p, m1, v1, sc)
    out = {"m": _score(m1, m_ref, m_abs, torch.isfinite(m_ref)), "v": _score(v1, v_ref, v_abs, torch.isfinite(v_ref)),
           "p": _score(p1, p_ref, p_abs, torch.isfinite(p_ref))}
    # where the reference is finite the implementation must be too (a NaN compares false with everything)
    for k, got, ref in (("m", m1, m_ref), ("v", v1, v_ref), ("p", p1, p_ref)):
        if bool((torch.isfinite(ref) & ~torch.isfinite(got)).any()):
            out[k] = float("inf")
    out["nonfinite"] = tuple(~torch.isfinite(x) for x in (p1, m1, v1))
    return out


def assert_adam_bounds(scores, where=""):
    for k in ("m", "v", "p"):
        assert scores[k] <= ADAM_K[k], (where, k, scores[k], "bound", ADAM_K[k])


def adam_gradients(n, gen, lo=1e-30, hi=1e4, zero_frac=0.05):
    """log-uniform magnitudes over [lo, hi], both signs, exact zeros"""
    e = torch.rand(n, generator=gen, dtype=torch.float64) * (math.log10(hi) - math.log10(lo)) + math.log10(lo)
    g = (10.0 ** e) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    g[torch.rand(n, generator=gen) < zero_frac] = 0.0
    return g.float()


def adam_state(n, gen, m_kind, v_kind):
    """the moment regimes: m zero / random, v zero / denormal (1e-40) / ordinary / 1e8"""
    m = torch.zeros(n) if m_kind == "zero" else torch.randn(n, generator=gen) * 0.1
    if v_kind == "zero":
        v = torch.zeros(n)
    elif v_kind == "denormal":
        v = torch.full((n,), 1e-40)
    elif v_kind == "ordinary":
        v = torch.rand(n, generator=gen) * 1e-2 + 1e-8
    else:
        v = torch.full((n,), 1e8)
    assert v_kind != "denormal" or (float(v[0]) > 0 and float(v[0]) < TINY)
    return m, v


M_KINDS, V_KINDS = ("zero", "random"), ("zero", "denormal", "ordinary", "1e8")
STEPS, EPSS = (1, 2, 1000, 30000, 1000000), (1e-8, 1e-15)


# ---- loss ------------------------------------------------------------------------------------------------------------
PAD = (loss_oracle.KERNEL_SIZE - 1) // 2
SHAPES = ((11, 11), (11, 48), (48, 11), (16, 16), (17, 33), (21, 27), (26, 42), (32, 64), (37, 53), (75, 131))
REGIMES = ("noise", "converged", "bright_flat", "out_of_range", "zero_background", "checkerboard")


def _consts(data_range=1.0):
    return (loss_oracle.K1 * data_range) ** 2, (loss_oracle.K2 * data_range) ** 2


def _ssim_from_moments(mx, my, exx, eyy, exy):
    c1, c2 = _consts()
    mu_x_sq, mu_y_sq, mu_xy = mx.pow(2), my.pow(2), mx * my
    s_xx, s_yy, s_xy = exx - mu_x_sq, eyy - mu_y_sq, exy - mu_xy
    return ((2 * mu_xy + c1) * (2 * s_xy + c2)) / ((mu_x_sq + mu_y_sq + c1) * (s_xx + s_yy + c2))


def ssim_map_2d(image, target):
    """loss_oracle.ssim's lines, returning the map [C, H - 10, W - 10] instead of its mean"""
    x = image.permute(2, 0, 1).unsqueeze(0)
    y = target.permute(2, 0, 1).unsqueeze(0)
    c = x.shape[1]
    g = loss_oracle.gaussian_kernel_1d(x.dtype)
    kernel = torch.matmul(g.t(), g).expand(c, 1, loss_oracle.KERNEL_SIZE, loss_oracle.KERNEL_SIZE)
    xp = F.pad(x, (PAD, PAD, PAD, PAD), mode="reflect")
    yp = F.pad(y, (PAD, PAD, PAD, PAD), mode="reflect")
    maps = torch.cat((xp, yp, xp * xp, yp * yp, xp * yp))
    out = F.conv2d(maps, kernel, groups=c).split(1)
    full = _ssim_from_moments(*out)
    return full[0, :, PAD:-PAD, PAD:-PAD]


def _row_then_column(a, g):
    """valid 11x11 window sums of a [C, H, W], row pass then column pass, tap by tap"""
    k = g.numel()
    Wv, Hv = a.shape[2] - k + 1, a.shape[1] - k + 1
    h = g[0] * a[:, :, 0:Wv]
    for j in range(1, k):
        h = h + g[j] * a[:, :, j:j + Wv]
    o = g[0] * h[:, 0:Hv]
    for i in range(1, k):
        o = o + g[i] * h[:, i:i + Hv]
    return o


def ssim_map_sep(image, target, mutate=None):
    """the same formula over the valid windows only, separable summation.  mutate (for the sensitivity test): "dxy"
    drops the y conv(D_xy) term of the gradient; "crop" counts one more column of windows than lie inside the image
    (they read zeros beyond the right edge) while dividing by the true count"""
    x, y = image.permute(2, 0, 1), target.permute(2, 0, 1)
    n_true = x.shape[0] * (x.shape[1] - 2 * PAD) * (x.shape[2] - 2 * PAD)
    if mutate == "crop":
        x, y = F.pad(x, (0, 1)), F.pad(y, (0, 1))
    g = loss_oracle.gaussian_kernel_1d(x.dtype)[0]
    xy = x.detach() * y if mutate == "dxy" else x * y
    m = _ssim_from_moments(*(_row_then_column(a, g) for a in (x, y, x * x, y * y, xy)))
    if mutate == "crop":
        m = m * (m.numel() / n_true)   # so that .mean() is the sum over one column too many divided by the true count
    return m


def loss_eval(image, target, frac, dtype, ssim_map=ssim_map_2d, **kw):
    """trainer.py:363-374 with the maps in `dtype` on the CPU -> dict(loss, l1, ssim, mse: floats; grad [H, W, 3]; map).
    The scalars are formed as the kernel forms them: the per-element terms summed in double, each mean rounded to
    `dtype`, the loss combined in `dtype` (in float64 these are loss_oracle's lines)"""
    img = image.to(dtype).clone().requires_grad_(True)
    tgt = target.to(dtype)
    smap = ssim_map(img, tgt, **kw)
    diff = img - tgt
    l1 = diff.abs().double().mean().to(dtype)
    s = smap.double().mean().to(dtype)
    mse = (diff * diff).detach().double().mean().to(dtype)
    loss = (1.0 - frac) * l1 + frac * (1.0 - s)
    grad, = torch.autograd.grad(loss, img)
    return dict(loss=float(loss.detach()), l1=float(l1.detach()), ssim=float(s.detach()), mse=float(mse), grad=grad.detach(),
                map=smap.detach())


def neighbourhood_env(env):
    """env [H, W, 3] >= 0 -> per pixel its maximum over the 21x21 neighbourhood and the channels, [H, W, 1]"""
    e = env.abs().amax(dim=2)[None, None]
    return F.max_pool2d(e, 4 * PAD + 1, stride=1, padding=2 * PAD)[0, 0].unsqueeze(2)


def grad_r(got, ref, env_nbhd):
    """max over pixels and channels of |got - ref| / (env_nbhd + 2^-22 |ref| + 1e-7 max|ref|)"""
    got, ref = got.detach().double().cpu(), ref.double()
    den = env_nbhd.double() + 2.0 ** -22 * ref.abs() + 1e-7 * ref.abs().max()
    num = (got - ref).abs()
    return float(torch.where(num == 0, torch.zeros_like(num), num / den).max())


def make_case(regime, H, W, seed=0):
    """-> image, target [H, W, 3] fp32 (the references see the fp32 values)"""
    gen = torch.Generator().manual_seed(1000 * H + W + 7919 * seed + 104729 * REGIMES.index(regime))
    rand = lambda: torch.rand(H, W, 3, generator=gen, dtype=torch.float64)
    randn = lambda: torch.randn(H, W, 3, generator=gen, dtype=torch.float64)
    if regime == "noise":
        image, target = rand(), rand()
    elif regime in ("converged", "out_of_range"):
        t = F.avg_pool2d(F.pad(rand().permute(2, 0, 1)[None], (3, 3, 3, 3), mode="replicate"), 7, stride=1)[0]
        t = t.permute(1, 2, 0)
        target = (t - t.min()) / (t.max() - t.min())
        image = target + 0.01 * randn() if regime == "converged" else 1.9 * target - 0.3 + 0.05 * randn()
    elif regime == "bright_flat":
        target = torch.full((H, W, 3), 0.9, dtype=torch.float64)
        image = 0.9 + 1e-3 * randn()
    elif regime == "zero_background":
        image, target = torch.zeros(H, W, 3, dtype=torch.float64), torch.zeros(H, W, 3, dtype=torch.float64)
        ys, xs = zero_background_block(H, W)
        image[ys, xs], target[ys, xs] = rand()[ys, xs], rand()[ys, xs]
    else:
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        image = ((yy + xx) % 2).double()[:, :, None].expand(H, W, 3).clone()
        target = 1.0 - image
    return image.float().contiguous(), target.float().contiguous()


def zero_background_block(H, W):
    """the central block (at most 5x5) outside which both images are exactly 0"""
    return slice(H // 2 - 2, H // 2 + 3), slice(W // 2 - 2, W // 2 + 3)


def far_from_block(H, W):
    """[H, W] bool: the pixels none of whose windows reaches the block (more than 10 pixels from it): every term
    of the gradient there is an exact zero"""
    ys, xs = zero_background_block(H, W)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    dy = torch.maximum(ys.start - yy, yy - (ys.stop - 1)).clamp(min=0)
    dx = torch.maximum(xs.start - xx, xx - (xs.stop - 1)).clamp(min=0)
    return torch.maximum(dy, dx) > 2 * PAD


@functools.lru_cache(maxsize=None)
def loss_reference(regime, H, W, frac=0.2):
    """the case, its float64 reference, the fp32 2-D restatement and the bounds of the scalars (factor 1).
    frac is rounded to fp32 as the C ABI's float argument rounds it.  Computed once per case; do not modify."""
    image, target = make_case(regime, H, W)
    f = f32(frac)
    ref = loss_eval(image, target, f, torch.float64)
    r32 = loss_eval(image, target, f, torch.float32)
    env = neighbourhood_env((r32["grad"].double() - ref["grad"]).abs())
    map_err = float((r32["map"].double() - ref["map"]).abs().mean())
    # l1: fl(x - y) per term (2^-24 of each |term|, so of their sum), the sum itself in double, the mean rounded to
    # fp32 once: 2 roundings.  mse: the squared rounded difference doubles the first, the product adds one: 4.
    b_l1 = 2.0 ** -23 * ref["l1"] + TINY
    b_mse = 2.0 ** -22 * ref["mse"] + TINY
    return dict(image=image, target=target, frac=f, ref=ref, fp32=r32, env=env, map_err=map_err, b_l1=b_l1, b_mse=b_mse)


def loss_scores(case, k, got_loss, got_l1, got_ssim, got_mse, got_grad):
    """the implementation's errors: "r" of the gradient and "ssim" in units of mean|map32 - map64| after the 2^-23
    allowance (both bounded by k); "l1", "mse" and "loss" in units of their bounds (the loss's taken with factor k)"""
    ref, f = case["ref"], case["frac"]
    e_ssim = abs(got_ssim - ref["ssim"])
    over = max(0.0, e_ssim - 2.0 ** -23)
    b_loss = (1.0 - f) * case["b_l1"] + f * (k * case["map_err"] + 2.0 ** -23) + 2.0 ** -23 * abs(ref["loss"])
    return dict(r=grad_r(got_grad, ref["grad"], case["env"]),
                ssim=0.0 if over == 0 else (over / case["map_err"] if case["map_err"] > 0 else float("inf")),
                l1=abs(got_l1 - ref["l1"]) / case["b_l1"], mse=abs(got_mse - ref["mse"]) / case["b_mse"],
                loss=abs(got_loss - ref["loss"]) / b_loss)


def assert_loss_bounds(sc, k, where=""):
    """k = 8 for the kernel, 4 for the separable fp32 restatement (the condition on the choice of inputs)"""
    assert sc["r"] <= k, (where, "gradient r", sc["r"])
    assert sc["ssim"] <= k, (where, "ssim", sc["ssim"])
    for name in ("l1", "mse", "loss"):
        assert sc[name] <= 1.0, (where, name, sc[name])
