"""The opt-in fused optimizer step: gs_preprocess_backward_adam (the per-Gaussian backward that applies Adam to
quaternion, scale, opacity, rgb and sh where their gradients are in registers) and train_ops.FusedRasterAdam on top
of it.  The kernel is checked for EQUALITY against the two calls it replaces (gs_preprocess_backward + gs_adam_step:
one shared definition of the arithmetic, no contraction); the wiring against an unfused frame on clones."""
import ctypes

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.densify import DensifyConfig, DensityController
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene
from gaussian_splatting_amd.train_ops import Adam, FusedRasterAdam, accumulate_grad_stats, ssim_l1_loss

from .helpers import scaled_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
FIVE = NAMES[1:]
# config.py of the reference: base_lr 0.002 times the per-group multipliers (tests/test_gpu_train_ops.py::LRS)
LRS = dict(xyz=0.002 * 0.1, quaternion=0.002 * 2, scale=0.002 * 5, opacity=0.002 * 10, rgb=0.002 * 2, sh=0.002 * 0.1)
STEPS = dict(quaternion=1, scale=2, opacity=7, rgb=1000, sh=3)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
ARGS = dict(near_thresh=0.3, far_thresh=500.0, cull_mask_padding=100, mh_dist=3.0, use_sh_precompute=True)


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off) if t is not None else None


def names_of(g):
    return [k for k in NAMES if getattr(g, k) is not None]


def build(optim_cls, g, **extra):
    """one group per tensor in the reference's order (optimizer_manager.py:15-42)"""
    opt = optim_cls([{"params": getattr(g, k), "lr": LRS[k]} for k in NAMES[:5]], **extra)
    if g.sh is not None:
        opt.add_param_group({"params": g.sh, "lr": LRS["sh"]})
    return opt


def kernel_case(N, n_sh, seed):
    """a frame's per-Gaussian forward, a random render-gradient slab and random starting moments"""
    deg = {1: 0, 4: 1, 9: 2, 16: 3}[n_sh]
    W, H = 256, 192
    g, cam, T = make_scene(N, W, H, deg, seed=seed, device=DEV)
    # near / far / padding that cull (z ~ U(1.5, 30); a sixth of the centres per axis lie outside the image)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, 2.0, 25.0, 20, 3.0,
                                 None, 0)
    V = f.V
    assert 0 < V < N   # culled Gaussians are part of every case
    gen = torch.Generator().manual_seed(seed + 1)
    slab = (torch.randn(V, 9, generator=gen) * 0.1).to(DEV)
    tensors = {}
    for k in FIVE:
        p = getattr(g, k)
        if p is None:
            continue
        m = (torch.randn(p.shape, generator=gen) * 0.01).to(DEV)
        v = (torch.rand(p.shape, generator=gen) * 1e-4).to(DEV)   # exp_avg_sq >= 0
        tensors[k] = (p.detach().clone(), m, v)
    return g, cam, T, f, slab, tensors


def run_reference(g, T, cam, f, slab, tensors):
    """gs_preprocess_backward, then gs_adam_step over the five tensors: -> grad_xyz, the gradients, stepped clones"""
    grads = fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab)
    by_name = dict(zip(("xyz", "quaternion", "scale", "opacity", "rgb", "sh"), grads))
    out = {k: tuple(t.clone() for t in tensors[k]) for k in tensors}
    ks = list(out)
    n = len(ks)
    arr = lambda i: (ctypes.c_void_p * n)(*[out[k][i].data_ptr() for k in ks])
    _hip.call("gs_adam_step", n, arr(0), (ctypes.c_void_p * n)(*[by_name[k].data_ptr() for k in ks]), arr(1), arr(2),
              (ctypes.c_int64 * n)(*[out[k][0].numel() for k in ks]), (ctypes.c_double * n)(*[LRS[k] for k in ks]),
              (ctypes.c_int64 * n)(*[STEPS[k] for k in ks]), ctypes.c_double(BETA1), ctypes.c_double(BETA2),
              ctypes.c_double(EPS), _hip.current_stream())
    return by_name, out


def call_fused(g, T, cam, f, slab, rows, steps=STEPS):
    """rows: {name: (p, m, v)} -- updated in place; -> grad_xyz"""
    grad_xyz = torch.full((f.N, 3), float("nan"), device=DEV)
    args = []
    for k in FIVE:
        p, m, v = rows.get(k, (None, None, None))
        args += [_p(p), _p(m), _p(v), ctypes.c_double(LRS[k]), ctypes.c_int64(steps[k])]
    _hip.call("gs_preprocess_backward_adam", _p(g.xyz), f.n_sh, _p(T), _p(cam.K), _p(f.center), _p(f.rank),
              _p(f.opacity_act), _p(slab), 0, f.N, _p(grad_xyz), *args, ctypes.c_double(BETA1), ctypes.c_double(BETA2),
              ctypes.c_double(EPS), _hip.current_stream())
    return grad_xyz


def adam_step_with_zero_gradient(k, p, m, v):
    """gs_adam_step on copies of the given rows with an all-zero gradient"""
    p, m, v = p.clone(), m.clone(), v.clone()
    zero = torch.zeros_like(p)
    one = lambda x: (ctypes.c_void_p * 1)(x.data_ptr())
    _hip.call("gs_adam_step", 1, one(p), one(zero), one(m), one(v), (ctypes.c_int64 * 1)(p.numel()),
              (ctypes.c_double * 1)(LRS[k]), (ctypes.c_int64 * 1)(STEPS[k]), ctypes.c_double(BETA1), ctypes.c_double(BETA2),
              ctypes.c_double(EPS), _hip.current_stream())
    return p, m, v


@pytest.mark.parametrize("N", [1000, 4099, 20000])
@pytest.mark.parametrize("n_sh", [1, 4, 9, 16])
def test_fused_kernel_equals_backward_then_adam_step(N, n_sh):
    """param, exp_avg, exp_avg_sq of all five tensors and grad_xyz: torch.equal between the fused kernel and
    gs_preprocess_backward + gs_adam_step, with a different lr and step count per tensor; culled rows equal an Adam
    step with gradient 0; xyz is untouched"""
    g, cam, T, f, slab, tensors = kernel_case(N, n_sh, seed=100 + n_sh)
    xyz_before = g.xyz.clone()
    # the fused kernel steps the frame's own quaternion / scale (inputs of the gradient and outputs of the step)
    grads, ref = run_reference(g, T, cam, f, slab, tensors)
    rows = {k: tuple(t.clone() for t in tensors[k]) for k in tensors}
    grad_xyz = call_fused(g, T, cam, f, slab, rows)
    torch.cuda.synchronize()
    assert torch.equal(grad_xyz, grads["xyz"])
    assert torch.equal(g.xyz, xyz_before)
    for k in tensors:
        for what, a, b in zip(("param", "exp_avg", "exp_avg_sq"), rows[k], ref[k]):
            assert torch.equal(a, b), (k, what, int((a != b).sum()), float((a - b).abs().max()))
    culled = f.culling_mask
    assert 0 < int(culled.sum()) < N
    for k in tensors:
        p0, m0, v0 = tensors[k]
        assert not grads[k][culled].any(), k
        p1, m1, v1 = adam_step_with_zero_gradient(k, p0[culled].contiguous(), m0[culled].contiguous(),
                                                  v0[culled].contiguous())
        assert torch.equal(rows[k][1][culled], m1), k
        assert torch.equal(rows[k][2][culled], v1), k
        assert torch.equal(rows[k][0][culled], p1), k
        assert not torch.equal(rows[k][0][culled], p0[culled]), k   # and they did move


def test_fused_kernel_unaligned_sh_views_take_the_scalar_path():
    """sh and its moments given as views at a 4-byte offset: same bits, the element in front of each view untouched"""
    N, n_sh = 4099, 16
    g, cam, T, f, slab, tensors = kernel_case(N, n_sh, seed=77)
    grads, ref = run_reference(g, T, cam, f, slab, tensors)
    rows = {k: tuple(t.clone() for t in tensors[k]) for k in tensors}
    stores = []
    views = []
    for t in tensors["sh"]:
        store = torch.full((t.numel() + 1,), 123.25, device=DEV)
        view = store[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0
        stores.append(store)
        views.append(view)
    rows["sh"] = tuple(views)
    grad_xyz = call_fused(g, T, cam, f, slab, rows)
    torch.cuda.synchronize()
    assert torch.equal(grad_xyz, grads["xyz"])
    for k in tensors:
        for what, a, b in zip(("param", "exp_avg", "exp_avg_sq"), rows[k], ref[k]):
            assert torch.equal(a, b), (k, what)
    assert all(float(s[0]) == 123.25 for s in stores)


def test_fused_kernel_refuses_bad_arguments():
    g, cam, T, f, slab, tensors = kernel_case(1000, 4, seed=5)
    rows = {k: tuple(t.clone() for t in tensors[k]) for k in tensors}
    before = {k: tuple(t.clone() for t in rows[k]) for k in rows}
    with pytest.raises(RuntimeError):
        call_fused(g, T, cam, f, slab, rows, steps=dict(STEPS, scale=0))   # the count AFTER the step is >= 1
    no_sh = {k: rows[k] for k in rows if k != "sh"}
    with pytest.raises(RuntimeError):
        call_fused(g, T, cam, f, slab, no_sh)   # n_sh > 1 without sh
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for k in rows for a, b in zip(rows[k], before[k]))


def fresh_scene(N, W, H, deg, seed):
    g, cam, T = make_scene(N, W, H, deg, seed=seed, device=DEV)
    for k in names_of(g):
        getattr(g, k).requires_grad_(True)
    return g, cam, T


@pytest.mark.parametrize("native", [False, True])
@pytest.mark.parametrize("deg", [0, 3])
def test_one_iteration_steps_five_tensors_in_the_backward(deg, native):
    N, W, H = 20000, 640, 472
    bg = torch.full((3,), 0.25, device=DEV)
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(8)).to(DEV)
    fused.NATIVE = native
    try:
        if native:
            assert fused.native() is not None and hasattr(fused.native(), "rasterize_adam")
        # the unfused frame on clones: the gradients the fused step must have used
        g0, cam, T = fresh_scene(N, W, H, deg, seed=2)
        img0, _, _ = fused.rasterize(g0, T, cam, background_rgb=bg, **ARGS)
        ssim_l1_loss(img0, target, 0.2).backward()
        g, cam, T = fresh_scene(N, W, H, deg, seed=2)
        names = names_of(g)
        start = {k: getattr(g, k).detach().clone() for k in names}
        opt = build(FusedRasterAdam, g)
        assert opt.fused_plan(g, True) is not None
        img, culled, uv = opt.rasterize(g, T, cam, background_rgb=bg, **ARGS)
        uv.retain_grad()
        assert torch.equal(img.detach(), img0.detach())
        ssim_l1_loss(img, target, 0.2).backward()
    finally:
        fused.NATIVE = True
    five = [k for k in FIVE if k in names]
    assert uv.grad is not None and g.xyz.grad is not None
    assert torch.equal(g.xyz.detach(), start["xyz"])
    assert scaled_err(g.xyz.grad, g0.xyz.grad) < 1e-5
    assert len(opt.state[g.xyz]) == 0
    for k in five:
        p = getattr(g, k)
        assert p.grad is None, k
        st = opt.state[p]
        assert float(st["step"]) == 1, k
        m, v = st["exp_avg"], st["exp_avg_sq"]
        # zero starting moments: exp_avg / (1 - beta1) is the gradient the kernel used
        err = scaled_err(m / (1.0 - BETA1), getattr(g0, k).grad)
        print(f"deg {deg} native {native} {k}: gradient scaled_err {err:.3g}")
        assert err < 1e-5, (k, err)
        # the parameter from the kernel's own moments, recomputed in torch (fp64)
        m_hat = m.double() / (1.0 - BETA1)
        v_hat = v.double() / (1.0 - BETA2)
        expect = start[k].double() - LRS[k] * m_hat / (v_hat.sqrt() + EPS)
        perr = float((p.detach().double() - expect).abs().max() / expect.abs().max())
        print(f"deg {deg} native {native} {k}: parameter error {perr:.3g} of max|p|")
        assert perr < 2e-6, (k, perr)
        assert not torch.equal(p.detach(), start[k]), k
    after_backward = {k: getattr(g, k).detach().clone() for k in five}
    opt.step()
    assert not torch.equal(g.xyz.detach(), start["xyz"])
    for k in five:
        assert torch.equal(getattr(g, k).detach(), after_backward[k]), k
    assert all(float(opt.state[getattr(g, k)]["step"]) == 1 for k in names)
    # the next iteration: step 2 for the five, and for xyz after step()
    opt.zero_grad(set_to_none=True)
    img, culled, uv = opt.rasterize(g, T, cam, background_rgb=bg, **ARGS)
    ssim_l1_loss(img, target, 0.2).backward()
    opt.step()
    assert all(float(opt.state[getattr(g, k)]["step"]) == 2 for k in names)
    assert all(torch.isfinite(getattr(g, k)).all() for k in names)


@pytest.mark.parametrize("case", ["weight_decay", "betas", "no_grad", "per_pixel_sh"])
def test_fallbacks_keep_the_unfused_results(case):
    N, W, H = 5000, 320, 240
    bg = torch.zeros(3, device=DEV)
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(9)).to(DEV)
    g, cam, T = fresh_scene(N, W, H, 1, seed=4)
    names = names_of(g)
    opt = build(FusedRasterAdam, g)
    args = dict(ARGS)
    if case == "weight_decay":
        opt.param_groups[2]["weight_decay"] = 0.01
    elif case == "betas":
        opt.param_groups[4]["betas"] = (0.8, 0.999)
    elif case == "per_pixel_sh":
        args["use_sh_precompute"] = False
    start = {k: getattr(g, k).detach().clone() for k in names}
    if case == "no_grad":
        with torch.no_grad():
            assert opt.fused_plan(g, True) is None
            img, culled, uv = opt.rasterize(g, T, cam, background_rgb=bg, **args)
            ref, _, _ = fused.rasterize(g, T, cam, background_rgb=bg, **args)
        assert not img.requires_grad and torch.equal(img, ref)
        opt.step()   # nothing has a gradient: nothing moves
        assert all(torch.equal(getattr(g, k).detach(), start[k]) for k in names)
        return
    assert opt.fused_plan(g, args["use_sh_precompute"]) is None
    img, culled, uv = opt.rasterize(g, T, cam, background_rgb=bg, **args)
    ssim_l1_loss(img, target, 0.2).backward()
    assert all(getattr(g, k).grad is not None for k in names)
    assert all(torch.equal(getattr(g, k).detach(), start[k]) for k in names)
    assert all(len(opt.state[getattr(g, k)]) == 0 for k in names)
    # train_ops.Adam on clones fed the same gradients
    g2, _, _ = fresh_scene(N, W, H, 1, seed=4)
    ref_opt = build(Adam, g2)
    for i, group in enumerate(opt.param_groups):
        for key in ("weight_decay", "betas"):
            ref_opt.param_groups[i][key] = group[key]
    for k in names:
        getattr(g2, k).grad = getattr(g, k).grad.clone()
    opt.step()
    ref_opt.step()
    for k in names:
        assert torch.equal(getattr(g, k).detach(), getattr(g2, k).detach()), k
        assert not torch.equal(getattr(g, k).detach(), start[k]), k


def test_a_second_consumer_of_a_stepped_parameter_is_caught():
    N, W, H = 5000, 320, 240
    bg = torch.zeros(3, device=DEV)
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(9)).to(DEV)
    g, cam, T = fresh_scene(N, W, H, 0, seed=4)
    opt = build(FusedRasterAdam, g)
    img, culled, uv = opt.rasterize(g, T, cam, background_rgb=bg, **ARGS)
    loss = ssim_l1_loss(img, target, 0.2) + 1e-3 * g.scale.exp().mean()   # a regulariser on scale
    loss.backward()
    assert g.scale.grad is not None and g.quaternion.grad is None
    with pytest.raises(RuntimeError, match="scale"):
        opt.step()


def test_training_iterations_reduce_the_loss_with_the_fused_step():
    """tests/test_gpu_train_ops.py::test_training_iterations_reduce_the_loss with FusedRasterAdam and opt.rasterize:
    same assertions, same thresholds"""
    N, W, H = 4000, 192, 128
    args = dict(near_thresh=0.3, far_thresh=500.0, cull_mask_padding=100, mh_dist=3.0, use_sh_precompute=True,
                background_rgb=torch.zeros(3, device=DEV))
    g, cam, T = make_scene(N, W, H, 1, seed=11, device=DEV)
    with torch.no_grad():
        target, _, _ = fused.rasterize(g, T, cam, **args)
        gen = torch.Generator().manual_seed(3)
        g.rgb.add_(0.5 * torch.randn(g.rgb.shape, generator=gen).to(DEV))
        g.xyz.add_(0.02 * torch.randn(g.xyz.shape, generator=gen).to(DEV))
    for k in NAMES:
        getattr(g, k).requires_grad_(True)
    opt = build(FusedRasterAdam, g)
    uv_acc, xyz_acc = torch.zeros(N, 2, device=DEV), torch.zeros(N, 3, device=DEV)
    count = torch.zeros(N, dtype=torch.int32, device=DEV)
    losses = []
    for it in range(40):
        opt.zero_grad(set_to_none=True)
        img, culled, uv = opt.rasterize(g, T, cam, **args)
        uv.retain_grad()
        loss = ssim_l1_loss(img, target, 0.2)
        loss.backward()
        assert all(getattr(g, k).grad is None for k in FIVE) and g.xyz.grad is not None
        opt.step()
        accumulate_grad_stats(uv.grad, culled, g.xyz.grad, cam, uv_acc, xyz_acc, count)
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.6 * losses[0], (losses[0], losses[-1])
    assert int(count.max()) == 40 and float(uv_acc.sum()) > 0 and torch.isfinite(xyz_acc).all()
    assert all(float(opt.state[getattr(g, k)]["step"]) == 40 for k in NAMES)


def test_the_fused_step_survives_density_control():
    """adaptive density control, an opacity reset and SH growth swap the parameters between iterations: the iteration
    after each still takes the fused step, with a fresh state entry / a restarted step count where the controller
    restarts it"""
    N, W, H = 30000, 320, 240
    g, cam, T = make_scene(N, W, H, 0, seed=2, device=DEV)
    for k in names_of(g):
        getattr(g, k).requires_grad_(True)
    opt = build(FusedRasterAdam, g)
    ctrl = DensityController(g, opt, DensifyConfig(adaptive_control_start=0, adaptive_control_end=100))
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    bg = torch.zeros(3, device=DEV)
    expect = {k: 0 for k in NAMES}
    sizes, events = [], []
    for it in range(1, 36):
        opt.zero_grad(set_to_none=True)
        img, culled, uv = opt.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
        uv.retain_grad()
        ssim_l1_loss(img, target, 0.2).backward()
        names = names_of(g)
        for k in names:
            expect[k] += 1
        for k in names[1:]:
            assert getattr(g, k).grad is None, (it, k)   # stepped in the backward, also right after a swap
            assert float(opt.state[getattr(g, k)]["step"]) == expect[k], (it, k)
        opt.step()
        assert float(opt.state[g.xyz]["step"]) == expect["xyz"]
        ctrl.accumulate(uv.grad, culled, cam)
        if it % 10 == 0:
            info = ctrl.adaptive_density_control(it)
            sizes.append(info["n_after"])
            events.append("density")
            assert g.xyz.shape[0] == info["n_after"]
        if it == 15:
            ctrl.reset_opacity()
            expect["opacity"] = 0   # _swap(restart=True)
            events.append("reset")
        if it in (20, 25):
            had = g.sh is not None
            ctrl.add_sh_band()
            if had:
                expect["sh"] = 0    # grown: zero moments and a restarted count
            events.append("sh")
    assert events.count("density") >= 1 and "reset" in events and events.count("sh") == 2
    assert g.sh is not None and g.sh.shape[2] == 8 and len(set(sizes)) > 1
    assert all(torch.isfinite(getattr(g, k)).all() for k in names_of(g))
