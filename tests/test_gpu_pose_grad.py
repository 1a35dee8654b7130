"""camera_T_world's gradient from the fused frame: gs_pose_backward (k_pose_bwd + k_pose_sum) at the stage level and
through both orchestrations of fused.rasterize, against the closed form of tests/pose_terms.py.

Error measure (pose_terms.pose_r), per element of the [3, 4] block: r = |got - sum t64| / (E + 2^-22 B) with t64 / t32
the closed-form terms of the visible Gaussians evaluated on the CPU in float64 / float32, B = sum |t64| and
E = sum |t32 - t64|; asserted max r <= 8 (R_MAX of test_gpu_general_cameras.py).  A frame's gradient is checked against
the slab it was computed from (fused.keep_last_slab): the render backward's summation order differs between runs.

Measured r on an MI355X (every case prints its r and leaves it in the parity report):
  stage: landscape N 200 1.45, odd N 777 0.86, landscape N 3000 deg 3 1.16, portrait N 70 000 0.43, one_tile_wide
  N 300 0.95; conic columns only 0.89, uv columns only 0.36
  frames (default / python / native): image loss 0.53 / 0.54 / 0.54, translation against A @ sum xyz.grad 0.018 /
  0.037 / 0.018, uv loss 0.10 / 0.10 / 0.10; tile_rows (3, 9) 0.89; depth cut 0.0035; the fused optimizer frame is
  compared with torch.equal.  The N = 600 000 stage case was added after that run: no figure recorded yet."""
import functools
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import make_grad_image, make_scene
from gaussian_splatting_amd.train_ops import FusedRasterAdam

from .helpers import report
from .pose_terms import pose_r, pose_reference
from .ref64 import general_camera_scene, random_slab, to_device

pytestmark = pytest.mark.gpu
DEV = "cuda"
R_MAX = 8.0
PARAMS = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")


def reference_of(g, T, K, culling_mask, slab):
    """(sum t64, B, E) of the Gaussians the frame kept, from CPU copies of its inputs and its slab"""
    vis = torch.nonzero(~culling_mask.cpu()).flatten()
    assert tuple(slab.shape) == (vis.numel(), 9), (slab.shape, vis.numel())
    c = lambda x: x.detach().cpu()
    return pose_reference(c(g.xyz)[vis], c(g.quaternion)[vis], c(g.scale)[vis], c(T), c(K), c(slab))


def check(tag, grad, ref, B, E):
    assert tuple(grad.shape) == (4, 4) and bool(torch.isfinite(grad).all()), tag
    assert not grad[3].any(), tag
    r = pose_r(grad, ref, B, E)
    report(tag, r=r, cancellation=float((ref.abs() / B.clamp(min=1e-300)).min()))
    print(f"{tag}: r = {r:.3g}")
    assert r <= R_MAX, (tag, r)


@functools.lru_cache(maxsize=None)
def stage_case(N, kind, deg):
    """a scene's per-Gaussian forward, a random slab and the closed form's reference (computed once per case)"""
    sc = general_camera_scene(80 + deg, N, deg=deg, kind=kind, stress=True)
    g, cam, T = to_device(sc, DEV)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, sc.near,
                                 sc.far, sc.pad, sc.mh, None, 0)
    assert 0 < f.V < N
    slab = random_slab(f.V, 17)
    return SimpleNamespace(sc=sc, g=g, cam=cam, T=T, f=f, slab=slab, ref=reference_of(g, T, cam.K, f.culling_mask, slab))


def stage_grad(c, slab):
    return fused.pose_backward(c.g.xyz, c.g.quaternion, c.g.scale, c.T, c.cam.K, c.f, slab.to(DEV).contiguous())


# N = 200: one partial workgroup; 70 000: more than 256 workgroup rows for the second level; 600 000: beyond
# 2048 x 256 = 524 288 Gaussians the grid is capped and a thread takes several Gaussians (what workload D runs on)
@pytest.mark.parametrize("N,kind,deg", [(200, "landscape", 0), (777, "odd", 1), (3000, "landscape", 3),
                                        (70_000, "portrait", 0), (300, "one_tile_wide", 2), (600_000, "landscape", 0)])
def test_stage_against_the_closed_form(N, kind, deg):
    c = stage_case(N, kind, deg)
    a = stage_grad(c, c.slab)
    b = stage_grad(c, c.slab)
    check(f"pose_stage[{kind} N {N} deg {deg}]", a, *c.ref)
    assert torch.equal(a, b)


@pytest.mark.parametrize("columns", ["conic", "uv"])
def test_stage_terms_one_at_a_time(columns):
    """a slab with only the conic columns, one with only the uv columns: a missing term cannot hide behind the other"""
    c = stage_case(777, "odd", 1)
    slab = torch.zeros_like(c.slab)
    sl = fused.SLAB_CONIC if columns == "conic" else fused.SLAB_UV
    slab[:, sl] = c.slab[:, sl]
    ref, B, E = reference_of(c.g, c.T, c.cam.K, c.f.culling_mask, slab)
    assert bool((B > 0).all())
    check(f"pose_stage[{columns} columns only]", stage_grad(c, slab), ref, B, E)


def test_stage_empty_frames_give_exact_zeros():
    sc = general_camera_scene(81, 777, kind="odd", stress=True)
    g, cam, T = to_device(sc, DEV)
    # far below every depth: nothing is visible
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, 0.1, 0.2,
                                 sc.pad, sc.mh, None, 0)
    assert f.V == 0
    slab = torch.ones(1, 9, device=DEV)
    got = fused.pose_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab)
    assert tuple(got.shape) == (4, 4) and not got.any()
    # N == 0
    e = lambda *s: torch.empty(*s, device=DEV)
    f0 = SimpleNamespace(N=0, rank=torch.empty(0, dtype=torch.int32, device=DEV))
    got = fused.pose_backward(e(0, 3), e(0, 4), e(0, 3), T, cam.K, f0, slab)
    assert tuple(got.shape) == (4, 4) and not got.any()


# ---- through fused.rasterize --------------------------------------------------------------------------------------
def frame_scene(N=3000, kind="odd", deg=1, seed=90):
    sc = general_camera_scene(seed, N, deg=deg, kind=kind, stress=True)
    g, cam, T = to_device(sc, DEV)
    for k in PARAMS:
        if getattr(g, k) is not None:
            getattr(g, k).requires_grad_(True)
    args = (sc.near, sc.far, sc.pad, sc.mh, True, torch.full((3,), 0.5, device=DEV))
    return sc, g, cam, T, args


def orchestration(mode):
    """-> the keyword arguments that select it"""
    if mode == "native" and fused.native() is None:
        pytest.skip("native frame module not built")
    return dict(frame_hook=lambda d: None) if mode == "python" else {}


@pytest.mark.parametrize("mode", ["default", "python", "native"])
def test_frame_gives_the_pose_its_gradient(mode):
    """517 x 301, 3000 Gaussians, loss = (image * w).sum(): camera_T_world.grad is the closed form of the frame's own
    slab, and its translation column agrees with A @ sum_g xyz.grad_g; then a loss on uv alone, whose slab is known"""
    kw = orchestration(mode)
    sc, g, cam, T, args = frame_scene()
    assert (sc.W, sc.H) == (517, 301)
    T.requires_grad_(True)
    w = make_grad_image(sc.W, sc.H, seed=4, device=DEV)
    fused.keep_last_slab(True)
    try:
        image, culling_mask, uv = fused.rasterize(g, T, cam, *args, **kw)
        (image * w).sum().backward()
        slab = fused.last_slab()
    finally:
        fused.keep_last_slab(False)
    assert T.grad is not None and tuple(T.grad.shape) == (4, 4) and bool(torch.isfinite(T.grad).all())
    assert slab is not None
    ref, B, E = reference_of(g, T, cam.K, culling_mask, slab)
    check(f"pose_frame[{mode}]", T.grad, ref, B, E)
    # dL/dt = sum_g g_cam and xyz.grad_g = A^T g_cam: for the scene's orthonormal A, A @ sum xyz.grad is dL/dt
    A = T.detach().double().cpu()[:3, :3]
    gx = g.xyz.grad.double().cpu()
    want = A @ gx.sum(0)
    Bx = A.abs() @ gx.abs().sum(0)
    num = (T.grad.double().cpu()[:3, 3] - want).abs()
    r = float((num / (E[:, 3] + 2.0 ** -22 * Bx)).max())
    report(f"pose_frame[{mode}] translation against xyz.grad", r=r)
    print(f"pose_frame[{mode}] translation against xyz.grad: r = {r:.3g}")
    assert r <= R_MAX
    # a loss on uv alone: the slab is (0 | 0 | w | 0) exactly
    T.grad = None
    image, culling_mask, uv = fused.rasterize(g, T, cam, *args, **kw)
    gen = torch.Generator().manual_seed(6)
    wu = torch.randn(uv.shape[0], 2, generator=gen)
    (uv * wu.to(DEV)).sum().backward()
    slab = torch.zeros(uv.shape[0], 9)
    slab[:, fused.SLAB_UV] = wu
    check(f"pose_frame[{mode}] uv loss", T.grad, *reference_of(g, T, cam.K, culling_mask, slab))


@pytest.mark.parametrize("mode", ["python", "native"])
def test_frame_without_a_pose_gradient_launches_nothing_new(mode):
    kw = orchestration(mode)
    sc, g, cam, T, args = frame_scene()
    w = make_grad_image(sc.W, sc.H, seed=4, device=DEV)
    calls = {}
    for want in (False, True):
        T.requires_grad_(want)
        _hip.enable_timing(True)
        try:
            image, _, _ = fused.rasterize(g, T, cam, *args, **kw)
            (image * w).sum().backward()
            calls[want] = _hip.collect_timing()
        finally:
            _hip.enable_timing(False)
    assert "gs_preprocess_backward" in calls[False] and "gs_pose_backward" not in calls[False]
    assert len(calls[True]["gs_pose_backward"]) == 1
    assert T.grad is not None


RASTER_MODES = {"classic": {}, "antialiased": dict(antialiased=True), "fisheye": dict(camera_model="fisheye")}
STEP_LABELS = ("gs_preprocess_forward", "gs_preprocess_backward", "gs_pose_backward")


@functools.lru_cache(maxsize=None)
def booked_frame(orch, raster):
    """One forward and one backward, under _hip.enable_timing, of a frame whose pose requires a gradient: 700 Gaussians
    (two whole 256-thread workgroups and a ragged third, some rows culled) on 517 x 301.  Computed once per case.
    The orchestration is chosen with fused.NATIVE: orchestration()'s frame_hook is refused by the antialiased and
    fisheye frames; it still skips the native case where the module is not built."""
    orchestration(orch)
    sc, g, cam, T, args = frame_scene(N=700)
    T.requires_grad_(True)
    w = make_grad_image(sc.W, sc.H, seed=4, device=DEV)
    prev = fused.NATIVE
    fused.NATIVE = orch == "native"
    fused.keep_last_slab(True)
    _hip.enable_timing(True)
    try:
        image, culling_mask, uv = fused.rasterize(g, T, cam, *args, **RASTER_MODES[raster])
        (image * w).sum().backward()
        booked = _hip.collect_timing()
        slab = fused.last_slab()
    finally:
        _hip.enable_timing(False)
        fused.keep_last_slab(False)
        fused.NATIVE = prev
    assert bool(culling_mask.any()) and not bool(culling_mask.all())
    grads = {k: getattr(g, k).grad for k in PARAMS}
    return SimpleNamespace(image=image.detach(), mask=culling_mask, slab=slab.contiguous(), grads=grads, pose=T.grad,
                           booked={k: len(v) for k, v in booked.items()})


@pytest.mark.parametrize("raster", list(RASTER_MODES))
@pytest.mark.parametrize("orch", ["python", "native"])
def test_one_general_call_per_step_in_every_mode(orch, raster):
    """Both orchestrations make one call per per-Gaussian step, to the general entry, and book it under the step's name
    in every mode; nothing is booked under a name ending in _mode.  The two orchestrations give the same image bit for
    bit.  Their gradients are compared through the slab each frame's own render backward left (its atomics' summation
    order differs from run to run, so two frames' gradients are not comparable directly): the six leaf gradients and
    the pose's are torch.equal to the per-Gaussian backward of that slab at the stage level -- one function of the
    slab for both orchestrations."""
    fr = booked_frame(orch, raster)
    for label in STEP_LABELS:
        assert fr.booked.get(label) == 1, (label, fr.booked)
    assert not [k for k in fr.booked if k.endswith("_mode")], fr.booked
    if fused.native() is not None:
        other = booked_frame("native" if orch == "python" else "python", raster)
        assert torch.equal(fr.image, other.image) and torch.equal(fr.mask, other.mask)
    sc, g, cam, T, args = frame_scene(N=700)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, sc.near,
                                 sc.far, sc.pad, sc.mh, None, 0, **RASTER_MODES[raster])
    assert f.V == fr.slab.shape[0] and 0 < f.V < 700
    with torch.no_grad():
        want = fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, fr.slab, **RASTER_MODES[raster])
        pose = fused.pose_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, fr.slab, **RASTER_MODES[raster])
    for k, wk in zip(PARAMS, want):
        assert bool(wk.any()) and torch.equal(fr.grads[k], wk), k
    assert bool(pose.any()) and torch.equal(fr.pose, pose)


def test_leaf_gradients_do_not_depend_on_the_pose_gradient():
    """the per-Gaussian node with and without a pose that requires grad, fed the same render gradients: the six leaf
    gradients are torch.equal"""
    c = stage_case(3000, "landscape", 3)
    sc = c.sc
    grads = {}
    for want in (False, True):
        g, cam, T = to_device(sc, DEV)
        leaves = [getattr(g, k).requires_grad_(True) for k in PARAMS]
        T.requires_grad_(want)
        uv, conic, opa, rgb = fused._Preprocess.apply(
            *leaves, T, cam.K, fused._frame_record(sc.W, sc.H, sc.near, sc.far, sc.pad, sc.mh, pose_grad=True))
        s = c.slab.to(DEV)
        torch.autograd.backward([uv, conic, opa, rgb], [s[:, fused.SLAB_UV], s[:, fused.SLAB_CONIC],
                                                        s[:, fused.SLAB_OPACITY], s[:, fused.SLAB_RGB]])
        grads[want] = [x.grad for x in leaves]
        assert (T.grad is not None) == want
    for k, a, b in zip(PARAMS, grads[False], grads[True]):
        assert a is not None and torch.equal(a, b), k
    check("pose_node[landscape N 3000 deg 3]", T.grad, *c.ref)


@pytest.mark.parametrize("mode", ["python", "native"])
def test_fused_optimizer_frame(mode):
    """FusedRasterAdam.rasterize with a pose that requires grad: the pose gradient is the one pose_backward gives on
    the PRE-step parameters and the same slab (the pose kernel runs before the step overwrites quaternion and scale),
    and the stepped parameters equal a fused step without a pose gradient on the same slab"""
    if mode == "native" and fused.native() is None:
        pytest.skip("native frame module not built")
    sc, g, cam, T, args = frame_scene()
    start = {k: getattr(g, k).detach().clone() for k in PARAMS}
    lrs = dict(xyz=2e-4, quaternion=4e-3, scale=1e-2, opacity=2e-2, rgb=4e-3, sh=2e-4)

    def optimizer(gg):
        return FusedRasterAdam([{"params": getattr(gg, k), "lr": lrs[k]} for k in PARAMS])

    opt = optimizer(g)
    T.requires_grad_(True)
    w = make_grad_image(sc.W, sc.H, seed=4, device=DEV)
    prev = fused.NATIVE
    fused.NATIVE = mode == "native"
    fused.keep_last_slab(True)
    try:
        image, culling_mask, uv = opt.rasterize(g, T, cam, *args)
        assert opt.last_fallback_reason is None
        (image * w).sum().backward()
        slab = fused.last_slab()
    finally:
        fused.keep_last_slab(False)
        fused.NATIVE = prev
    assert g.quaternion.grad is None and not torch.equal(g.quaternion.detach(), start["quaternion"])
    # the same slab at the stage level, on clones of the pre-step parameters
    g2, cam2, T2 = to_device(sc, DEV)
    for k in PARAMS:
        getattr(g2, k).copy_(start[k])
        getattr(g2, k).requires_grad_(True)
    f = fused.preprocess_forward(g2.xyz, g2.quaternion, g2.scale, g2.opacity, g2.rgb, g2.sh, T2, cam2.K, sc.W, sc.H,
                                 sc.near, sc.far, sc.pad, sc.mh, None, 0)
    assert f.V == slab.shape[0]
    want = fused.pose_backward(g2.xyz, g2.quaternion, g2.scale, T2, cam2.K, f, slab.contiguous())
    assert torch.equal(T.grad, want)
    plan = optimizer(g2).fused_plan(g2, True)
    assert plan is not None
    with torch.no_grad():
        grad_xyz = fused.preprocess_backward_adam(g2.xyz, T2, cam2.K, f, slab.contiguous(), plan)
    assert torch.equal(g.xyz.grad, grad_xyz)
    for k in PARAMS[1:]:
        assert torch.equal(getattr(g, k).detach(), getattr(g2, k).detach()), k


def test_tile_rows_frame():
    sc, g, cam, T, args = frame_scene()
    T.requires_grad_(True)
    w = make_grad_image(sc.W, sc.H, seed=4, device=DEV)
    fused.keep_last_slab(True)
    try:
        image, culling_mask, uv = fused.rasterize(g, T, cam, *args, tile_rows=(3, 9))
        (image * w).sum().backward()
        slab = fused.last_slab()
    finally:
        fused.keep_last_slab(False)
    check("pose_frame[tile_rows (3, 9)]", T.grad, *reference_of(g, T, cam.K, culling_mask, slab))


def test_depth_cut_frame():
    """a frame that takes the depth-bucketed binning (forced; lists of ~1800 entries per tile) uses the same node"""
    N, W, H = 90_000, 256, 192
    g, cam, T = make_scene(N, W, H, 0, seed=9, device=DEV)
    g.opacity.fill_(-5.0)
    for k in PARAMS:
        if getattr(g, k) is not None:
            getattr(g, k).requires_grad_(True)
    T.requires_grad_(True)
    w = make_grad_image(W, H, seed=3, device=DEV)
    prev = fused.DEPTH_CUT
    fused.DEPTH_CUT = True
    fused.keep_last_slab(True)
    try:
        before = fused.counters()["depth_cut_frames"]
        image, culling_mask, uv = fused.rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, torch.full((3,), 0.25, device=DEV))
        (image * w).sum().backward()
        slab = fused.last_slab()
        assert fused.counters()["depth_cut_frames"] == before + 1
    finally:
        fused.keep_last_slab(False)
        fused.DEPTH_CUT = prev
    check("pose_frame[depth cut]", T.grad, *reference_of(g, T, cam.K, culling_mask, slab))
