"""tests/train_ref64.py held to PyTorch's own float64 results on the CPU, and correct fp32 implementations shown to
meet the bounds that tests/test_gpu_train_ref64.py puts on the kernels.

Adam: the reference chained over 5 steps equals torch.optim.Adam on float64 tensors; torch.optim.Adam in fp32 meets
the stage-wise bounds on every regime of the GPU test (measured here: m' 1.8, v' 1.9, p' 4.2 at most, in
units of 2^-24 abs_sum; bounds 4 / 5 / 7).
Loss: the float64 evaluation equals oracle/loss_oracle.py and passes gradcheck; on every case of the GPU test the
separable fp32 restatement (another summation order) stays within HALF the kernel's bounds against the 2-D
restatement's envelope -- the condition on the choice of inputs (measured: r 1.14 at most, in bright_flat); a restatement with one of two plausible kernel bugs
scores far beyond the bound."""
import pytest
import torch

from oracle import loss_oracle

from . import train_ref64 as T

BETAS = (0.9, 0.999)


# ---- Adam ------------------------------------------------------------------------------------------------------------
def test_adam_reference_equals_torch_adam_in_float64():
    gen = torch.Generator().manual_seed(0)
    n, lr, eps = 2000, 0.004, 1e-8
    p = torch.randn(n, generator=gen).double().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=BETAS, eps=eps)
    rp, rm, rv = p.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        g = T.adam_gradients(n, gen, lo=1e-6, hi=1e2).double()
        p.grad = g.clone()
        opt.step()
        # the reference rounds its scalars to fp32 (that is the kernel's contract); here they stay doubles
        sc = dict(w1=1.0 - BETAS[0], beta2=BETAS[1], w2=1.0 - BETAS[1], eps=eps,
                  neg_step=-(lr / (1.0 - BETAS[0] ** step)), bc2_sqrt=(1.0 - BETAS[1] ** step) ** 0.5)
        (rm, _), (rv, _) = T.adam_moments(g, rm, rv, sc)
        rp, _ = T.adam_param(rp, rm, rv, sc)
    st = opt.state[p]
    for name, got, want in (("p", rp, p.detach()), ("m", rm, st["exp_avg"]), ("v", rv, st["exp_avg_sq"])):
        err = float((got - want).abs().max() / want.abs().max())
        assert err <= 1e-14, (name, err)


def test_adam_scalars_round_as_the_kernel_does():
    sc = T.adam_scalars(0.004, 3, 0.9, 0.999, 1e-15)
    for k, v in sc.items():
        assert v == float(torch.tensor(v, dtype=torch.float32)), k          # representable in fp32
    assert sc["neg_step"] == T.f32(-(0.004 / (1.0 - 0.9 ** 3))) and sc["eps"] == T.f32(1e-15) and sc["eps"] > 0


def _torch_adam_fp32(p, g, m, v, lr, step, eps):
    q = p.clone().requires_grad_(True)
    q.grad = g.clone()
    opt = torch.optim.Adam([q], lr=lr, betas=BETAS, eps=eps)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    st = opt.state[q]
    assert float(st["step"]) == step
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("m_kind", T.M_KINDS)
@pytest.mark.parametrize("v_kind", T.V_KINDS)
def test_torch_adam_in_fp32_meets_the_stagewise_bounds(m_kind, v_kind):
    n = 20000
    gen = torch.Generator().manual_seed(11 + 7 * T.M_KINDS.index(m_kind) + T.V_KINDS.index(v_kind))
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for i, (step, eps) in enumerate((s, e) for s in T.STEPS for e in T.EPSS):
        lr = T.LRS[(i + T.V_KINDS.index(v_kind)) % len(T.LRS)]
        p, g = torch.randn(n, generator=gen), T.adam_gradients(n, gen)
        m, v = T.adam_state(n, gen, m_kind, v_kind)
        after = _torch_adam_fp32(p, g, m, v, lr, step, eps)
        sc = T.adam_scores((p, g, m, v), after, lr, step, *BETAS, eps)
        T.assert_adam_bounds(sc, (step, eps, lr))
        worst = {k: max(worst[k], sc[k]) for k in worst}
    print("torch fp32 Adam, units of 2^-24 abs_sum:", m_kind, v_kind, worst)


def test_adam_bounds_notice_a_wrong_step():
    """the measure is not vacuous: a dropped bias correction in p', beta2 in the place of 1 - beta2 in v'"""
    n, lr, step, eps = 5000, 0.004, 2, 1e-8
    gen = torch.Generator().manual_seed(3)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-3
    m, v = T.adam_state(n, gen, "random", "ordinary")
    sc = T.adam_scalars(lr, step, *BETAS, eps)
    (m1, _), (v1, _) = T.adam_moments(g, m, v, sc)
    m1, v1 = m1.float(), v1.float()
    good = T.adam_param(p, m1, v1, sc)[0].float()
    T.assert_adam_bounds(T.adam_scores((p, g, m, v), (good, m1, v1), lr, step, *BETAS, eps))
    no_bc2 = (p.double() + sc["neg_step"] * m1.double() / (v1.double().sqrt() + sc["eps"])).float()
    assert T.adam_scores((p, g, m, v), (no_bc2, m1, v1), lr, step, *BETAS, eps)["p"] > T.ADAM_K["p"]
    v_bad = (v.double() * sc["beta2"] + sc["beta2"] * g.double() * g.double()).float()
    assert T.adam_scores((p, g, m, v), (good, m1, v_bad), lr, step, *BETAS, eps)["v"] > T.ADAM_K["v"]


# ---- loss ------------------------------------------------------------------------------------------------------------
def test_loss_reference_is_the_oracle_in_float64():
    image, target = T.make_case("converged", 37, 53)
    for frac in (0.0, 0.2, 1.0):
        x = image.double().requires_grad_(True)
        loss, l1, s = loss_oracle.ssim_l1_loss(x, target.double(), frac)
        loss.backward()
        ref = T.loss_eval(image, target, frac, torch.float64)
        assert abs(ref["loss"] - float(loss.detach())) <= 1e-15 and abs(ref["l1"] - float(l1.detach())) <= 1e-15
        assert abs(ref["ssim"] - float(s.detach())) <= 1e-15
        assert float((ref["grad"] - x.grad).abs().max()) <= 1e-15 * float(x.grad.abs().max())


def test_ssim_gradcheck_in_float64():
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(12, 13, 3, generator=gen, dtype=torch.float64).requires_grad_(True)
    y = torch.rand(12, 13, 3, generator=gen, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda a: loss_oracle.ssim(a, y), (x,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_separable_restatement_equals_the_reference_in_float64():
    """valid windows only + another summation order is the same function: 1e-12 in float64"""
    for regime in T.REGIMES:
        image, target = T.make_case(regime, 21, 27)
        a = T.loss_eval(image, target, 0.2, torch.float64)
        b = T.loss_eval(image, target, 0.2, torch.float64, T.ssim_map_sep)
        assert abs(a["ssim"] - b["ssim"]) <= 1e-12 and float((a["map"] - b["map"]).abs().max()) <= 1e-10
        assert float((a["grad"] - b["grad"]).abs().max()) <= 1e-11 * float(a["grad"].abs().max())


def _sep_scores(regime, H, W, frac, k, **kw):
    case = T.loss_reference(regime, H, W, frac)
    sep = T.loss_eval(case["image"], case["target"], case["frac"], torch.float32, T.ssim_map_sep, **kw)
    return T.loss_scores(case, k, sep["loss"], sep["l1"], sep["ssim"], sep["mse"], sep["grad"])


@pytest.mark.parametrize("regime", T.REGIMES)
def test_separable_fp32_restatement_stays_within_half_the_bound(regime):
    """the condition on the choice of inputs (every shape; ssim_frac 0.2, and 0 and 1 at two shapes)"""
    worst = {}
    for H, W in T.SHAPES:
        for frac in ((0.2, 0.0, 1.0) if (H, W) in ((17, 33), (37, 53)) else (0.2,)):
            sc = _sep_scores(regime, H, W, frac, T.R_MAX / 2)
            T.assert_loss_bounds(sc, T.R_MAX / 2, (regime, H, W, frac))
            worst = {k: max(worst.get(k, 0.0), v) for k, v in sc.items()}
    print("separable fp32 restatement:", regime, worst)


def test_zero_background_gradient_is_exactly_zero_in_the_reference():
    H, W = 37, 53
    case = T.loss_reference("zero_background", H, W)
    far = T.far_from_block(H, W)
    assert bool(far.any()) and not bool(far.all())
    assert not bool(case["ref"]["grad"][far].any()) and not bool(case["fp32"]["grad"][far].any())
    assert bool(case["ref"]["grad"][~far].any())


@pytest.mark.parametrize("regime", ["converged", "checkerboard"])
@pytest.mark.parametrize("bug", ["crop", "dxy"])
def test_measure_notices_plausible_kernel_bugs(regime, bug):
    """a window column too many counted at an edge; the y conv(D_xy) term of the gradient dropped"""
    sc = _sep_scores(regime, 37, 53, 0.2, T.R_MAX, mutate=bug)
    assert sc["r"] > T.R_MAX, sc


def test_fixed_tolerances_do_not_fit_a_bright_flat_region():
    """what DESIGN.md 7b records: the fp32 restatement's own error on 0.9 + 1e-3 N against 0.9 is far beyond the
    1e-5 / 1e-4 tolerances that suit uniform noise"""
    case = T.loss_reference("bright_flat", 37, 53)
    ref, r32 = case["ref"], case["fp32"]
    assert abs(r32["ssim"] - ref["ssim"]) > 1e-5
    assert float((r32["grad"].double() - ref["grad"]).abs().max() / ref["grad"].abs().max()) > 1e-4
    noise = T.loss_reference("noise", 37, 53)
    assert abs(noise["fp32"]["ssim"] - noise["ref"]["ssim"]) < 1e-5
