"""train_ops.FusedRasterAdam decides per frame whether the backward may take the fused optimizer step.  The decision
looks at the param groups and at tensor metadata only, so it is checked here without a device: CPU tensors and every
disqualifying group option give "fall back", each for its own reason."""
import pytest
import torch

from gaussian_splatting_amd.synthetic import make_scene
from gaussian_splatting_amd.train_ops import Adam, FusedRasterAdam

NAMES = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")


def scene_and_optimizer(deg=1, **extra):
    g, cam, T = make_scene(200, 64, 48, deg, seed=0)
    for k in NAMES:
        if getattr(g, k) is not None:
            getattr(g, k).requires_grad_(True)
    opt = FusedRasterAdam([{"params": getattr(g, k), "lr": 1e-3} for k in NAMES if getattr(g, k) is not None], **extra)
    return g, opt


def test_it_is_an_adam_with_the_same_state_layout():
    g, opt = scene_and_optimizer()
    assert isinstance(opt, Adam) and isinstance(opt, torch.optim.Adam)
    assert [grp["params"][0] for grp in opt.param_groups] == [getattr(g, k) for k in NAMES]


def test_cpu_tensors_fall_back_for_being_cpu_tensors():
    for deg in (0, 1):
        g, opt = scene_and_optimizer(deg)
        plan, why = opt.fused_decision(g, True)
        assert plan is None and why == "not fp32 device tensors"
        assert opt.fused_plan(g, True) is None and opt.last_fallback_reason == why


@pytest.mark.parametrize("option,value", [("amsgrad", True), ("weight_decay", 0.01), ("maximize", True),
                                          ("capturable", True), ("differentiable", True)])
@pytest.mark.parametrize("group", [1, 5])
def test_each_disqualifying_group_option_falls_back(option, value, group):
    g, opt = scene_and_optimizer()
    opt.param_groups[group][option] = value
    plan, why = opt.fused_decision(g, True)
    assert plan is None and option in why and NAMES[group] in why
    # the same option on xyz, which step() handles, does not decide anything here
    g, opt = scene_and_optimizer()
    opt.param_groups[0][option] = value
    assert opt.fused_decision(g, True) == (None, "not fp32 device tensors")


def test_the_other_conditions():
    g, opt = scene_and_optimizer()
    opt.param_groups[3]["betas"] = (0.8, 0.999)
    assert opt.fused_decision(g, True) == (None, "the groups do not share betas and eps")
    g, opt = scene_and_optimizer()
    opt.param_groups[2]["eps"] = 1e-6
    assert opt.fused_decision(g, True) == (None, "the groups do not share betas and eps")
    g, opt = scene_and_optimizer()
    assert "per-pixel SH" in opt.fused_decision(g, False)[1]
    with torch.no_grad():
        assert opt.fused_decision(g, True) == (None, "grad mode is off")
    # the groups must hold the very tensors of the Gaussians, in the reference's order
    g.scale = torch.nn.Parameter(g.scale.detach().clone())
    assert "'scale'" in opt.fused_decision(g, True)[1]
    g, opt = scene_and_optimizer(0)
    g2, _ = scene_and_optimizer(1)
    g.sh = g2.sh   # SH that the optimizer has no group for
    assert "no param group for 'sh'" == opt.fused_decision(g, True)[1]


def test_fallback_step_is_adams_step_on_the_cpu():
    """no device anywhere: rasterize is not called, step() is Adam.step (which hands CPU tensors to torch)"""
    g, opt = scene_and_optimizer()
    g2, ref = scene_and_optimizer()
    ref = torch.optim.Adam([{"params": getattr(g2, k), "lr": 1e-3} for k in NAMES])
    gen = torch.Generator().manual_seed(1)
    for k in NAMES:
        grad = torch.randn(getattr(g, k).shape, generator=gen)
        getattr(g, k).grad = grad.clone()
        getattr(g2, k).grad = grad.clone()
    opt.step()
    ref.step()
    assert all(torch.equal(getattr(g, k).detach(), getattr(g2, k).detach()) for k in NAMES)
