"""Normal maps and the normal-consistency regulariser (ABI 21): gs_gaussian_normals, gs_depth_normal and their
backwards against tests/normals_ref.py, fused.rasterize_normals as a frame, the pose, a short training run and the refusals.

Measures (imported, unchanged):
  stage kernels   ref64.r_measure against the float64 restatement with env = |its float32 evaluation - float64|,
                  bound R_MAX = 8 (tests/test_gpu_general_cameras.py).  Left out: the rows within FLIP_MARGIN of the flip
                  and the pixels whose cross product nearly vanishes (normals_ref; capped at 0.5 % on the CPU), and for the
                  depth gradients the pixels next to one of those.
  the frame       image / culling_mask / uv of rasterize, depth / alpha of rasterize_rgbd, normal_map of
                  rasterize_features fed gs_gaussian_normals' own output: equal to the bit, on the stage scenes at their
                  own sizes and once per mode.  The gradients of a loss on all four maps are held to the float64 chain
                  link by link: the kept slab and the gradient of the channels (last_grad_normals | last_grad_z) against
                  tests/features_ref.py on the kernel's normals under tests/test_gpu_render_ref64.py's noise rule and
                  margin (rule (b) and the combined slab of tests/test_gpu_features.py, whose helpers run here); the
                  normals' backward of that very gradient against normals_ref's float64 autograd by r_measure; and the
                  parameter gradients equal to fused.preprocess_backward of the kept slab plus those two terms, exactly.
                  That reference composites on the CPU pixel by pixel, so this one test runs on the 70 x 45 frame of
                  the render tests, as the feature frame's does.
  the pose        tests/pose_terms.py's pose_r and bound, with the rotation term's |t64| and |t32 - t64| added to B, E
  plane           the device's normals of an exact plane within 40 * 2^-24 max|P| / min(|D_y P|, |D_x P|) of -m / |m|:
                  a back-projected point carries five roundings (depth and alpha as stored, the division, the ray, the
                  product), a difference of two twice that, and the normalised cross product of two nearly perpendicular
                  differences turns by at most the sum of their relative errors; a factor 2 for the cross product's own
                  roundings.

One deviation.  The float64-chain gradient test runs on the 70 x 45 frame, not on a stage scene (above); on the stage
scenes the gradients are only required to arrive at all six tensors, to be finite and, for the quaternion, to differ from
rasterize_rgbd's.

Measured on an MI355X (every case leaves its figures in the parity report):
  Gaussian normals   r 0.68 / 0.73 forward, 0.54 / 0.34 backward (landscape / odd); no row left out
  depth normals      r 0.84 to 1.07 on the normals, 0.74 to 0.99 on both gradients, both models, no pixel left out; with the
                     device library's tanf in the fisheye ray 66 at 517 x 301: the ray is now the kernel's
                     own sequence of +, *, / that normals_ref repeats
  wide fisheye       16 x 16 at f = 3 and 61 x 47 at f = 21: 179 / 93 pixels without a ray, 29 / 1411 valid beyond pi / 4;
                     r 0.98 / 1.0 on the normals, 0.87 to 1.0 on the gradients; without the envelope 5.1e-7 / 7.6e-6
                     against bounds of 1.3e-5 / 1.2e-4
  plane              5.1e-5 (bound 1.2e-3) at 517 x 301, 2.9e-6 (bound 8.8e-5) at 37 x 29
  frame chain        r_feature_map 2.0, r_alpha 2.1; slab and channel gradients 2.0e-6 .. 3.4e-6 against bounds of 2.4e-5 ..
                     3.3e-5; the normals' backward of the kept gradient r 0.60
  pose               r 0.84, the rotation term a third of the total; without the term 5.9e4
  training           loss 0.0353, 0.0216, 0.0153, 0.0128, 0.0121 at steps 0, 10, 20, 30, 40; mean angle 0.271 -> 0.139 rad
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused, train_ops
from gaussian_splatting_amd.splat_py.structs import Camera, Gaussians
from gaussian_splatting_amd.synthetic import DEFAULTS

from . import features_ref as F
from . import normals_ref as N
from .helpers import report
from .pose_terms import pose_r, pose_reference
from .ref64 import general_camera_scene, r_measure, random_slab, to_device
from .test_gpu_depth_alpha import BG, FRAME, PARAMS, fp32_fma_close, frame_inputs
from .test_gpu_features import check_rule, forward_measures, oracle_bounds
from .test_gpu_render_ref64 import NOISE_MARGIN, frame_reference, noise_measure
from .test_normals_ref import TAN_BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda"
R_MAX = 8.0
SENTINEL = -777.0
SLACK = 32
p = _hip.ptr


def check(tag, **rs):
    report(tag, **rs)
    print(tag, {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rs.items()})
    for k, v in rs.items():
        if k.startswith("r_"):
            assert v <= R_MAX, (tag, k, v)


# ---- 1. the Gaussians' normals ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_case(kind):
    sc = N.stage_scene(kind)
    g, cam, T = to_device(sc, DEV)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, sc.near,
                                 sc.far, sc.pad, sc.mh, None, 0)
    V = f.V
    assert 0 < V < N.N_STAGE
    vis = f.vis_idx[:V].long().cpu()
    rows = SimpleNamespace(q=sc.g.quaternion[vis], s=sc.g.scale[vis], p=f.xyz_cam[:V].cpu())
    n64, info = N.gaussian_normals(rows.q, rows.s, sc.T, rows.p, detail=True)
    return SimpleNamespace(sc=sc, g=g, cam=cam, T=T, f=f, V=V, vis=vis, rows=rows, n64=n64, info=info,
                           fragile=info.facing.abs() < N.FLIP_MARGIN)


@pytest.mark.parametrize("kind", list(N.STAGE_SCENES))
def test_gaussian_normals_forward_and_backward(kind):
    c = stage_case(kind)
    V, NN, ok = c.V, N.N_STAGE, ~c.fragile
    s = _hip.current_stream()
    # forward: nothing behind normals[V] is written
    buf = torch.full((V * 3 + SLACK,), SENTINEL, device=DEV)
    _hip.call("gs_gaussian_normals", p(c.g.quaternion), p(c.g.scale), p(c.T), p(c.f.vis_idx), p(c.f.xyz_cam), V, p(buf), s)
    got = buf[:V * 3].view(V, 3).cpu()
    assert bool((buf[V * 3:] == SENTINEL).all()) and bool(torch.isfinite(got).all())
    assert torch.equal(fused.gaussian_normals_forward(c.g.quaternion, c.g.scale, c.T, c.f.vis_idx[:V], c.f.xyz_cam).cpu(), got)
    n32 = N.gaussian_normals(c.rows.q, c.rows.s, c.sc.T, c.rows.p, torch.float32).double()
    # the flip the kernel took: the reference's wherever the decision is not fragile; every normal faces the camera
    flipped = (got.double() * torch.where(c.info.flip[:, None], -c.n64, c.n64)).sum(dim=1) < 0
    assert torch.equal(flipped[ok], c.info.flip[ok])
    assert bool(((got.double() * c.rows.p.double()).sum(dim=1)[ok] < 0).all())
    assert float((got.double().norm(dim=1) - 1).abs().max()) < 1e-5
    vals = dict(V=V, left_out=int(c.fragile.sum()), r_forward=r_measure(got[ok], c.n64[ok], (n32 - c.n64)[ok]))
    # the stress rows the kernel can get wrong are among the visible ones
    dense = torch.zeros(NN, dtype=torch.bool)
    dense[c.vis] = True
    for name in ("quat_norm", "log_scale", "needle_disc"):
        assert int(dense[c.sc.rows[name]].sum()) > 20, name
    # backward: every row of grad_quaternion written, culled rows exactly zero
    g_n = random_slab(V, 23)[:, :3].contiguous()
    gq = torch.full((NN, 4), SENTINEL, device=DEV)
    _hip.call("gs_gaussian_normals_backward", p(c.g.quaternion), p(c.g.scale), p(c.T), p(c.f.rank), p(c.f.xyz_cam),
              p(g_n.to(DEV)), V, NN, p(gq), s)
    gq = gq.cpu()
    assert not gq[~dense].any() and bool(torch.isfinite(gq).all()) and float(gq[dense].abs().max()) > 0
    ref = {}
    for dtype in (torch.float64, torch.float32):
        q = c.rows.q.detach().clone().to(dtype).requires_grad_(True)
        (N.gaussian_normals(q, c.rows.s, c.sc.T, c.rows.p, dtype) * g_n.to(dtype)).sum().backward()   # (rows are independent)
        ref[dtype] = q.grad.double()
    vals["r_backward"] = r_measure(gq[c.vis][ok], ref[torch.float64][ok], (ref[torch.float32] - ref[torch.float64])[ok])
    check(f"gaussian_normals[{kind}]", **vals)


def test_gaussian_normals_single_row_and_empty():
    q = torch.tensor([[2.0, 0.0, 0.0, 0.0]], device=DEV)
    sc = torch.tensor([[0.0, 0.0, -3.0]], device=DEV)
    T = torch.eye(4, device=DEV)
    pc = torch.tensor([[0.2, -0.1, 5.0]], device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    n = fused.gaussian_normals_forward(q, sc, T, idx, pc)
    assert torch.equal(n.cpu(), torch.tensor([[0.0, 0.0, -1.0]]))
    # ties: the lowest index; an exact 0 is not flipped
    n = fused.gaussian_normals_forward(q, torch.zeros(1, 3, device=DEV), T, idx, torch.tensor([[0.0, 1.0, 1.0]], device=DEV))
    assert torch.equal(n.cpu(), torch.tensor([[1.0, 0.0, 0.0]]))
    gq = fused.gaussian_normals_backward(q, sc, T, idx, pc, torch.tensor([[1.0, 2.0, 3.0]], device=DEV))
    # n = -R[:, 2] = -(2 (xz + yw), 2 (yz - xw), 1 - 2 (x^2 + y^2)) at qhat = (1, 0, 0, 0): d/dx = (0, 2, 0), d/dy = (-2, 0, 0)
    assert torch.allclose(gq.cpu(), torch.tensor([[0.0, 4.0, -2.0, 0.0]]) / 2.0)
    e = lambda *s: torch.empty(*s, device=DEV)
    assert fused.gaussian_normals_forward(q, sc, T, idx[:0], pc[:0]).shape == (0, 3)
    assert fused.gaussian_normals_backward(e(0, 4), e(0, 3), T, idx[:0], e(0, 3), e(0, 3)).shape == (0, 4)
    # nothing visible among N: all rows written as zeros
    rank = torch.full((5,), -1, dtype=torch.int32, device=DEV)
    out = torch.full((5, 4), SENTINEL, device=DEV)
    _hip.call("gs_gaussian_normals_backward", None, None, None, p(rank), None, None, 0, 5, p(out), _hip.current_stream())
    assert not out.any()


# ---- 2. the depth map's normal ------------------------------------------------------------------------------------------
MODELS = {"pinhole": False, "fisheye": True}


def grow(mask):
    """the pixels of mask and their four neighbours"""
    out = mask.clone()
    out[1:] |= mask[:-1]
    out[:-1] |= mask[1:]
    out[:, 1:] |= mask[:, :-1]
    out[:, :-1] |= mask[:, 1:]
    return out


def reference_maps(m, fisheye, min_alpha, g_n):
    """normals_ref's normal, validity, fragile pixels and, by autograd, the two gradients, in float64 and float32"""
    out = {}
    for dtype in (torch.float64, torch.float32):
        depth = m.depth.detach().clone().to(dtype).requires_grad_(True)
        alpha = m.alpha.detach().clone().to(dtype).requires_grad_(True)
        n, valid, fragile = N.depth_normal(depth, alpha, m.K, fisheye, min_alpha, dtype, detail=True)
        if n.requires_grad:
            (n * g_n.to(dtype)).sum().backward()
        zero = torch.zeros(m.H, m.W, dtype=torch.float64)
        out[dtype] = SimpleNamespace(n=n.detach().double(), valid=valid, fragile=fragile,
                                     g_depth=depth.grad.double() if depth.grad is not None else zero,
                                     g_alpha=alpha.grad.double() if alpha.grad is not None else zero)
    return out[torch.float64], out[torch.float32]


def device_maps(m, model, min_alpha, g_n):
    depth, alpha = m.depth.detach().to(DEV).requires_grad_(True), m.alpha.detach().to(DEV).requires_grad_(True)
    cam = Camera(m.W, m.H, m.K.to(DEV))
    n = fused.depth_to_normal(depth, alpha, cam, model, min_alpha)
    (n * g_n.to(DEV)).sum().backward()
    return n.detach().cpu(), depth.grad.cpu(), alpha.grad.cpu()


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("W,H", N.MAP_SIZES)
def test_depth_normal_forward_and_backward(W, H, model):
    fisheye = MODELS[model]
    m = N.depth_maps(W, H, fisheye)
    g_n = N.random_normal_grad(H, W, 31)
    r64, r32 = reference_maps(m, fisheye, 0.0, g_n)
    # every pixel of [H, W, 3] is written and nothing behind it
    buf = torch.full((H * W * 3 + SLACK,), SENTINEL, device=DEV)
    mode = _hip.GS_RASTER_FISHEYE if fisheye else _hip.GS_RASTER_CLASSIC
    d_dev, a_dev, K_dev = m.depth.to(DEV), m.alpha.to(DEV), m.K.to(DEV)
    _hip.call("gs_depth_normal", p(d_dev), p(a_dev), p(K_dev), W, H, 0.0, mode, p(buf), _hip.current_stream())
    assert bool((buf[H * W * 3:] == SENTINEL).all()) and not bool((buf[:H * W * 3] == SENTINEL).any())
    n, gd, ga = device_maps(m, model, 0.0, g_n)
    assert torch.equal(buf[:H * W * 3].view(H, W, 3).cpu(), n)
    assert bool(torch.isfinite(n).all()) and bool(torch.isfinite(gd).all()) and bool(torch.isfinite(ga).all())
    keep = ~r64.fragile
    got_valid = (n != 0).any(dim=2)
    assert torch.equal(got_valid[keep], r64.valid[keep])
    assert not n[m.zero_core].any()                       # the degenerate cross product: invalid, exactly zero
    sel = r64.valid & keep
    vals = dict(valid=float(r64.valid.float().mean()), left_out=int(r64.fragile.sum()))
    vals["r_normal"] = r_measure(n[sel], r64.n[sel], (r32.n - r64.n)[sel])
    if bool(sel.any()):
        assert float((n[sel].double().norm(dim=1) - 1).abs().max()) < 1e-5
    # the gradients: exactly zero where no valid centre's stencil holds the pixel; elsewhere the reference's
    near = ~grow(r64.fragile)
    untouched = ~grow(r64.valid) & near
    assert not gd[untouched].any() and not ga[untouched].any()
    for k, got in (("g_depth", gd), ("g_alpha", ga)):
        w64, w32 = getattr(r64, k), getattr(r32, k)
        vals[f"r_{k}"] = r_measure(got[near].reshape(-1, 1), w64[near].reshape(-1, 1), (w32 - w64)[near].reshape(-1, 1))
    if min(W, H) < 3:
        assert not n.any() and not gd.any() and not ga.any()
    else:
        assert float(gd.abs().max()) > 0 and float(ga.abs().max()) > 0
    # no atomics: a second run gives the same bits
    n2, gd2, ga2 = device_maps(m, model, 0.0, g_n)
    assert torch.equal(n2, n) and torch.equal(gd2, gd) and torch.equal(ga2, ga)
    check(f"depth_normal[{W}x{H} {model}]", **vals)


@pytest.mark.parametrize("W,H,f", N.WIDE_SIZES)
def test_depth_normal_wide_fisheye(W, H, f):
    """a short focal length: rays from the axis through pi / 4 (the other branch of tan_over_theta) to beyond 90 degrees
    (no ray: the pixel and every centre whose stencil holds it are invalid).  The assertions of the other maps, and
    exact zeros -- output and both gradients -- at and around the pixels without a ray"""
    m = N.wide_maps(W, H, f)
    g_n = N.random_normal_grad(H, W, 33)
    r64, r32 = reference_maps(m, True, 0.0, g_n)
    buf = torch.full((H * W * 3 + SLACK,), SENTINEL, device=DEV)
    d_dev, a_dev, K_dev = m.depth.to(DEV), m.alpha.to(DEV), m.K.to(DEV)
    _hip.call("gs_depth_normal", p(d_dev), p(a_dev), p(K_dev), W, H, 0.0, _hip.GS_RASTER_FISHEYE, p(buf), _hip.current_stream())
    assert bool((buf[H * W * 3:] == SENTINEL).all()) and not bool((buf[:H * W * 3] == SENTINEL).any())
    n, gd, ga = device_maps(m, "fisheye", 0.0, g_n)
    assert torch.equal(buf[:H * W * 3].view(H, W, 3).cpu(), n)
    assert bool(torch.isfinite(n).all()) and bool(torch.isfinite(gd).all()) and bool(torch.isfinite(ga).all())
    keep = ~r64.fragile
    assert torch.equal((n != 0).any(dim=2)[keep], r64.valid[keep])
    no_ray = ~m.ray_ok
    assert bool(no_ray.any()) and not n[grow(no_ray)].any()          # no ray: it and its four neighbours are invalid
    assert not gd[no_ray].any() and not ga[no_ray].any()             # ... and it belongs to no valid centre's stencil
    sel, near = r64.valid & keep, ~grow(r64.fragile)
    beyond = sel & (m.theta > N.PIO4)
    assert int(beyond.sum()) > 10
    vals = dict(valid=float(r64.valid.float().mean()), no_ray=int(no_ray.sum()), beyond_pi_4=int(beyond.sum()),
                left_out=int(r64.fragile.sum()), theta_max_valid=float(m.theta[sel].max()))
    vals["r_normal"] = r_measure(n[sel], r64.n[sel], (r32.n - r64.n)[sel])
    vals["r_normal_beyond_pi_4"] = r_measure(n[beyond], r64.n[beyond], (r32.n - r64.n)[beyond])
    untouched = ~grow(r64.valid) & near
    assert not gd[untouched].any() and not ga[untouched].any()
    for k, got in (("g_depth", gd), ("g_alpha", ga)):
        w64, w32 = getattr(r64, k), getattr(r32, k)
        vals[f"r_{k}"] = r_measure(got[near].reshape(-1, 1), w64[near].reshape(-1, 1), (w32 - w64)[near].reshape(-1, 1))
    assert float(gd[beyond].abs().max()) > 0 and float(ga[beyond].abs().max()) > 0
    # and without the envelope, which repeats the kernel's factor: between pi / 4 and 1.4 rad a back-projected point is
    # within TAN_BOUND (tests/test_normals_ref.py: the factor against float64) + five roundings of its true value, a
    # difference of two within twice that of max|P|, and the normalised cross product turns by at most the sum of the two
    # differences' relative errors (the plane test's reasoning, with its factor 2 for the cross product's own roundings)
    ray64, _ = N.rays(m.K, W, H, True, torch.float64)
    d64 = m.depth.double() / torch.where(m.alpha > 0, m.alpha, torch.ones_like(m.alpha)).double()
    P = d64[:, :, None] * ray64
    mid = beyond & ~grow(m.theta > 1.4)
    a = torch.zeros(H, W, dtype=torch.float64)
    b = torch.zeros(H, W, dtype=torch.float64)
    a[1:-1, 1:-1], b[1:-1, 1:-1] = (P[2:, 1:-1] - P[:-2, 1:-1]).norm(dim=2), (P[1:-1, 2:] - P[1:-1, :-2]).norm(dim=2)
    assert int(mid.sum()) > 10
    tol = 8 * (TAN_BOUND + 5 * 2.0 ** -24) * float(P[grow(mid)].norm(dim=1).max()) / float(torch.minimum(a, b)[mid].min())
    vals["beyond_pi_4_abs_error"], vals["beyond_pi_4_tol"] = float((n[mid].double() - r64.n[mid]).abs().max()), tol
    assert vals["beyond_pi_4_abs_error"] <= tol, vals
    n2, gd2, ga2 = device_maps(m, "fisheye", 0.0, g_n)
    assert torch.equal(n2, n) and torch.equal(gd2, gd) and torch.equal(ga2, ga)
    check(f"depth_normal_wide[{W}x{H} f {f}]", **vals)


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("W,H", [(37, 29), (517, 301)])
def test_depth_normal_min_alpha_and_plane(W, H, model):
    fisheye = MODELS[model]
    m = N.depth_maps(W, H, fisheye)
    g_n = N.random_normal_grad(H, W, 32)
    r0, _ = reference_maps(m, fisheye, 0.0, g_n)
    r64, r32 = reference_maps(m, fisheye, 0.5, g_n)
    assert int(r64.valid.sum()) < int(r0.valid.sum()) and bool(r64.valid.any())   # the threshold removes pixels
    n, gd, ga = device_maps(m, model, 0.5, g_n)
    keep = ~r64.fragile
    assert torch.equal((n != 0).any(dim=2)[keep], r64.valid[keep])
    sel, near = r64.valid & keep, ~grow(r64.fragile)
    vals = dict(r_normal=r_measure(n[sel], r64.n[sel], (r32.n - r64.n)[sel]))
    for k, got in (("g_depth", gd), ("g_alpha", ga)):
        w64, w32 = getattr(r64, k), getattr(r32, k)
        vals[f"r_{k}"] = r_measure(got[near].reshape(-1, 1), w64[near].reshape(-1, 1), (w32 - w64)[near].reshape(-1, 1))
    # the plane's known answer on the device
    alpha = (0.5 + 0.5 * torch.rand(H, W, generator=torch.Generator().manual_seed(1), dtype=torch.float64)).float()
    d = N.plane_depth(m.K, W, H, fisheye)
    plane = SimpleNamespace(depth=(d * alpha.double()).float().contiguous(), alpha=alpha, K=m.K, W=W, H=H)
    pn, _, _ = device_maps(plane, model, 0.0, g_n)
    ray, _ = N.rays(m.K, W, H, fisheye, torch.float64)
    P = d[:, :, None] * ray
    a, b = (P[2:, 1:-1] - P[:-2, 1:-1]).norm(dim=2), (P[1:-1, 2:] - P[1:-1, :-2]).norm(dim=2)
    tol = 40 * 2.0 ** -24 * float(P.norm(dim=2).max()) / float(torch.minimum(a, b).min())
    mhat = N.PLANE[0].double() / N.PLANE[0].double().norm()
    inner = pn[1:-1, 1:-1].double()
    vals["plane_error"], vals["plane_tol"] = float((inner + mhat).abs().max()), tol
    assert not pn[0].any() and not pn[-1].any() and not pn[:, 0].any() and not pn[:, -1].any()
    check(f"depth_normal_min_alpha_plane[{W}x{H} {model}]", **vals)
    assert vals["plane_error"] <= tol, vals


# ---- 3. the frame --------------------------------------------------------------------------------------------------------
FRAME_MODES = {"classic": {}, "antialiased": dict(antialiased=True), "fisheye": dict(camera_model="fisheye"),
               "filter3d": "filter3d"}


def stage_frame(kind, grads=True):
    sc = N.stage_scene(kind)
    g, cam, T = to_device(sc, DEV)
    if grads:
        for k in PARAMS:
            if getattr(g, k) is not None:
                getattr(g, k).requires_grad_(True)
    return sc, g, cam, T, (sc.near, sc.far, sc.pad, sc.mh, True, torch.full((3,), 0.5, device=DEV))


@pytest.mark.parametrize("kind,mode", [("landscape", "classic"), ("odd", "classic"), ("odd", "antialiased"),
                                       ("odd", "fisheye"), ("odd", "filter3d")])
def test_frame_is_the_other_frames_bit_for_bit(kind, mode):
    sc, g, cam, T, args = stage_frame(kind)
    kw = FRAME_MODES[mode]
    if kw == "filter3d":
        gen = torch.Generator().manual_seed(8)
        kw = dict(filter3d=(torch.exp(2 * sc.g.scale.min(dim=1).values) * torch.rand(N.N_STAGE, generator=gen)).to(DEV))
    image, depth, alpha, normal_map, mask, uv = fused.rasterize_normals(g, T, cam, *args, **kw)
    W, H = sc.W, sc.H
    assert tuple(normal_map.shape) == (H, W, 3) and tuple(depth.shape) == (H, W) and tuple(alpha.shape) == (H, W)
    with torch.no_grad():
        image0, mask0, uv0 = fused.rasterize(g, T, cam, *args, **kw)
        _, depth1, alpha1, _, _ = fused.rasterize_rgbd(g, T, cam, *args, **kw)
        assert torch.equal(image, image0) and torch.equal(mask, mask0) and torch.equal(uv, uv0)
        assert torch.equal(depth, depth1) and torch.equal(alpha, alpha1)
        # rasterize_features fed gs_gaussian_normals' own output (and z)
        f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, sc.near, sc.far,
                                     sc.pad, sc.mh, None, 0, camera_model=kw.get("camera_model", "pinhole"))
        V = f.V
        assert V == uv.shape[0] and V > 1000
        normals = fused.gaussian_normals_forward(g.quaternion, g.scale, T, f.vis_idx[:V], f.xyz_cam)
        feat = torch.zeros(N.N_STAGE, 4, device=DEV)
        feat[f.vis_idx[:V].long()] = torch.cat((normals, f.xyz_cam[:V, 2:3]), dim=1)
        _, fmap, alpha2, _, _ = fused.rasterize_features(g, feat, T, cam, *args, **kw)
        assert torch.equal(normal_map, fmap[..., :3]) and torch.equal(depth, fmap[..., 3]) and torch.equal(alpha, alpha2)
    assert float(normal_map.abs().max()) > 0.1 and float(alpha.max()) > 0.5
    # |sum w n| <= sum w |n| = alpha
    assert bool((normal_map.detach().norm(dim=2) <= alpha.detach() * (1 + 1e-5) + 1e-6).all())
    # a loss on all four maps reaches the six parameter tensors
    gen = torch.Generator().manual_seed(9)
    w = torch.randn(H, W, 8, generator=gen).to(DEV) / (W * H)
    ((image * w[..., :3]).sum() + (normal_map * w[..., 3:6]).sum() + (depth * w[..., 6]).sum()
     + (alpha * w[..., 7]).sum()).backward()
    # ... every one of them finite, and the quaternion's not the one rasterize_rgbd gives the same loss without the
    # normal map
    _, g1, _, _, _ = stage_frame(kind)
    image1, depth1, alpha1, _, _ = fused.rasterize_rgbd(g1, T, cam, *args, **kw)
    ((image1 * w[..., :3]).sum() + (depth1 * w[..., 6]).sum() + (alpha1 * w[..., 7]).sum()).backward()
    for k in PARAMS:
        t = getattr(g, k)
        if t is not None:
            assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0, k
    assert not torch.equal(g.quaternion.grad, g1.quaternion.grad)


@functools.lru_cache(maxsize=None)
def chain_case():
    """the 70 x 45 frame's own uv / conic / opacity and complete lists (a return_aux frame), the kernel's normals and z
    of its visible Gaussians as the four channels, the features reference on them for a seeded [g_N | g_depth | g_alpha]
    and rule (a)'s bounds"""
    shift = FRAME["shift"]
    g, cam, T, bg = frame_inputs(shift, grads=False)
    W, H = FRAME["W"], FRAME["H"]
    image, mask, uv, aux = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, return_aux=True, **DEFAULTS)
    cpu = lambda x: x.detach().cpu().contiguous()
    V = uv.shape[0]
    vis_idx = aux["vis_idx"][:V]
    xyz_cam = aux["xyz_camera_frame"][:V].contiguous()
    normals = fused.gaussian_normals_forward(g.quaternion, g.scale, T, vis_idx.contiguous(), xyz_cam)
    feat = torch.cat((normals, xyz_cam[:, 2:3]), dim=1)
    gen = torch.Generator().manual_seed(FRAME["seed"] + 5)
    base = SimpleNamespace(name=f"normals_frame{shift}", W=W, H=H, V=V, uv=cpu(uv), conic=cpu(aux["conic"]),
                           opacity=cpu(aux["opacity"]).reshape(V, 1), rays=torch.zeros(H, W, 3),
                           sorted_g=cpu(aux["sorted_gaussians"]).int(), ranges=cpu(aux["tile_ranges"]).int())
    sc = F.as_features_scene(base, cpu(feat), torch.randn(H, W, 5, generator=gen))
    ref = F.reference_of(sc, sc.g_all)
    scaled = ref.scale != 1
    true = F.reference_of(sc, sc.g_all * (~scaled)[:, :, None]) if bool(scaled.any()) else ref
    vals = {}
    orc, bounds = oracle_bounds(vals, sc, true)
    return SimpleNamespace(sc=sc, ref=ref, orc=orc, bounds=bounds, vals=vals, image=cpu(image), mask=cpu(mask), uv=cpu(uv),
                           vis_idx=cpu(vis_idx).long(), xyz_cam=cpu(xyz_cam), shift=shift)


def test_frame_gradients_against_the_float64_chain():
    case = chain_case()
    sc, ref, shift = case.sc, case.ref, case.shift
    W, H, NN = sc.W, sc.H, FRAME["N"]
    csc, cref, corc = frame_reference()
    assert torch.equal(csc.uv, sc.uv) and torch.equal(csc.sorted_g, sc.sorted_g)
    g, cam, T, bg = frame_inputs(shift)
    fused.keep_last_slab(True)
    try:
        _hip.set_backward_mode("exact")
        image, depth, alpha, normal_map, mask, uv = fused.rasterize_normals(g, T, cam, use_sh_precompute=True,
                                                                            background_rgb=bg, **DEFAULTS)
        gi = ref.grad_image.float().to(DEV)
        torch.autograd.backward([normal_map, depth, alpha, image],
                                [gi[..., :3].contiguous(), gi[..., 3].contiguous(), gi[..., 4].contiguous(),
                                 cref.grad_image.float().to(DEV)])
        slab, g_z, g_n = fused.last_slab(), fused.last_grad_z(), fused.last_grad_normals()
    finally:
        _hip.set_backward_mode("compat")
        fused.keep_last_slab(False)
    assert torch.equal(image.detach().cpu(), case.image) and torch.equal(mask.cpu(), case.mask)
    assert torch.equal(uv.detach().cpu(), case.uv)
    assert slab is not None and g_z is not None and g_n is not None
    assert tuple(slab.shape) == (sc.V, 9) and tuple(g_z.shape) == (sc.V,) and tuple(g_n.shape) == (sc.V, 3)
    # the render's link: forward rule, then the slab and the channels' gradient under the noise rule
    ok = ~ref.fragile
    fmap = torch.cat((normal_map.detach(), depth.detach()[..., None]), dim=2).cpu()
    vals = dict(case.vals, V=sc.V, fragile=float(ref.fragile.float().mean()))
    vals.update(forward_measures(dict(feature_map=fmap, alpha=alpha.detach().cpu()), case.orc, ref, ok))
    cs = slab.cpu()
    got = dict(g_features=torch.cat((g_n, g_z[:, None]), dim=1).cpu(), g_opacity=cs[:, fused.SLAB_OPACITY],
               g_uv=cs[:, fused.SLAB_UV], g_conic=cs[:, fused.SLAB_CONIC])
    bounds = dict(case.bounds)
    want = SimpleNamespace(grad=dict(ref.grad), abs=dict(ref.abs), used=ref.used | cref.used)
    for k in F.SHARED:
        want.grad[k] = ref.grad[k] + cref.grad_walk[k]
        want.abs[k] = ref.abs[k] + cref.abs_walk[k]
        bounds[k] = max(bounds[k], noise_measure(corc[k], cref.grad_walk[k], cref.abs_walk[k]) + NOISE_MARGIN)
    verdict_f = check_rule(vals, "b", got, SimpleNamespace(grad=ref.grad, abs=ref.abs, used=ref.used), bounds,
                           keys=("g_features",))
    verdict = check_rule(vals, "b", got, want, bounds, keys=F.SHARED)
    # the normals' link: the backward of that very gradient against the float64 autograd of the restatement
    cq = lambda x: x.detach().cpu()
    q_v, s_v = cq(g.quaternion)[case.vis_idx], cq(g.scale)[case.vis_idx]
    _, info = N.gaussian_normals(q_v, s_v, cq(T), case.xyz_cam, detail=True)
    keep = info.facing.abs() >= N.FLIP_MARGIN
    chain = {}
    for dtype in (torch.float64, torch.float32):
        q = q_v.detach().clone().to(dtype).requires_grad_(True)
        (N.gaussian_normals(q, s_v, cq(T), case.xyz_cam, dtype) * cq(g_n).to(dtype)).sum().backward()   # (rows are independent)
        chain[dtype] = q.grad.double()
    g2, cam2, T2, _ = frame_inputs(shift, grads=False)
    rec = fused.preprocess_forward(g2.xyz, g2.quaternion, g2.scale, g2.opacity, g2.rgb, g2.sh, T2, cam2.K, W, H,
                                   DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"],
                                   DEFAULTS["mh_dist"], None, 0)
    assert rec.V == sc.V and torch.equal(rec.xyz_cam[:rec.V].cpu(), case.xyz_cam)
    gqn = fused.gaussian_normals_backward(g2.quaternion, g2.scale, T2, rec.rank, rec.xyz_cam, g_n.contiguous())
    vals["r_normals_backward"] = r_measure(gqn.cpu()[case.vis_idx][keep], chain[torch.float64][keep],
                                           (chain[torch.float32] - chain[torch.float64])[keep])
    report("normals_frame_chain", **vals)
    print("normals_frame_chain", vals)
    assert vals["r_feature_map"] <= R_MAX and vals["r_alpha"] <= R_MAX and vals["r_normals_backward"] <= R_MAX, vals
    verdict_f()
    verdict()
    # the per-Gaussian node: the kept slab through fused.preprocess_backward on a fresh record, plus the two terms
    gx, gq, gs, go, gc, gsh = fused.preprocess_backward(g2.xyz, g2.quaternion, g2.scale, T2, cam2.K, rec, slab.contiguous())
    for k, w in (("scale", gs), ("opacity", go), ("rgb", gc)):
        assert torch.equal(getattr(g, k).grad, w), k
    assert torch.equal(g.quaternion.grad, gq + gqn) or torch.equal(g.quaternion.grad, gqn + gq)
    assert float(gqn.abs().max()) > 0
    rank = rec.rank.cpu().long()
    vis = rank >= 0
    z_term = torch.zeros(NN, 3, dtype=torch.float64)
    z_term[vis] = g_z.double().cpu()[rank[vis]][:, None] * T2.double().cpu()[2, :3][None, :]
    assert fp32_fma_close(g.xyz.grad, gx, z_term)


def test_frame_with_nothing_visible():
    g, cam, T, bg = frame_inputs(0.0)
    T.requires_grad_(True)
    image, depth, alpha, normal_map, mask, uv = fused.rasterize_normals(g, T, cam, 0.1, 0.2, 100, 3.0, True, bg)
    assert uv.shape[0] == 0 and bool(mask.all())
    assert tuple(normal_map.shape) == (FRAME["H"], FRAME["W"], 3) and not normal_map.any() and not depth.any()
    assert not alpha.any() and bool((image == BG).all())
    (normal_map.sum() + depth.sum() + alpha.sum() + image.sum()).backward()
    for k in PARAMS:
        t = getattr(g, k)
        assert t is None or t.grad is None or not t.grad.any(), k
    assert T.grad is None or not T.grad.any()


# ---- 4. the pose -----------------------------------------------------------------------------------------------------------
def test_pose_gradient_of_a_normal_map_loss():
    """517 x 301, 3000 Gaussians, camera_T_world requires grad, the loss reads normal_map only: T.grad against the closed
    form of tests/pose_terms.py on the kept slab plus the float64 sum of the direct term of n_c = +-W n_w on the kept
    gradient of the normals (dL/dW += sum g (x) +-n_w); pose_r with that term's |t64| and |t32 - t64| added to B and E"""
    sc = general_camera_scene(90, 3000, deg=1, kind="odd", stress=True)
    g, cam, T = to_device(sc, DEV)
    for k in PARAMS:
        getattr(g, k).requires_grad_(True)
    T.requires_grad_(True)
    bg = torch.full((3,), 0.5, device=DEV)
    w = torch.randn(sc.H, sc.W, 3, generator=torch.Generator().manual_seed(4)).to(DEV) / (sc.W * sc.H)
    fused.keep_last_slab(True)
    try:
        image, depth, alpha, normal_map, mask, uv = fused.rasterize_normals(g, T, cam, sc.near, sc.far, sc.pad, sc.mh, True, bg)
        (normal_map * w).sum().backward()
        slab, g_n, g_z = fused.last_slab(), fused.last_grad_normals(), fused.last_grad_z()
    finally:
        fused.keep_last_slab(False)
    assert slab is not None and g_n is not None and not slab[:, :3].any()
    assert g_z is None or not g_z.any()           # the depth channel had no gradient
    vis = torch.nonzero(~mask.cpu()).flatten()
    c = lambda x: x.detach().cpu()
    q_v, s_v, xyz_v = c(g.quaternion)[vis], c(g.scale)[vis], c(g.xyz)[vis]
    ref, B, E = pose_reference(xyz_v, q_v, s_v, c(T), c(cam.K), c(slab))
    slab_only = ref.clone()
    # the flip of each row as the frame took it: from its own normals (a fragile row's may differ from float64's)
    f = fused.preprocess_forward(g.xyz.detach(), g.quaternion.detach(), g.scale.detach(), g.opacity.detach(),
                                 g.rgb.detach(), g.sh.detach(), T.detach(), cam.K, sc.W, sc.H, sc.near, sc.far, sc.pad,
                                 sc.mh, None, 0)
    p_cam = f.xyz_cam[:f.V].cpu()
    got_n = fused.gaussian_normals_forward(g.quaternion.detach(), g.scale.detach(), T.detach(), f.vis_idx[:f.V], f.xyz_cam).cpu()
    terms = {}
    for dtype in (torch.float64, torch.float32):
        _, info = N.gaussian_normals(q_v, s_v, c(T), p_cam, dtype, detail=True)
        unflipped = info.n_world.to(dtype) @ c(T).to(dtype)[:3, :3].t()
        sign = torch.where((got_n.to(dtype) * unflipped).sum(dim=1) < 0, -1.0, 1.0).to(dtype)
        t = torch.zeros(vis.numel(), 3, 4, dtype=dtype)
        t[:, :, :3] = c(g_n).to(dtype)[:, :, None] * (sign[:, None] * info.n_world.to(dtype))[:, None, :]
        terms[dtype] = t.double()
    t64, t32 = terms[torch.float64], terms[torch.float32]
    ref, B, E = ref + t64.sum(0), B + t64.abs().sum(0), E + (t32 - t64).abs().sum(0)
    assert T.grad is not None and tuple(T.grad.shape) == (4, 4) and bool(torch.isfinite(T.grad).all())
    assert not T.grad[3].any()
    r = pose_r(T.grad, ref, B, E)
    share = float((t64.sum(0).abs()[:, :3] / ref.abs()[:, :3].clamp(min=1e-300)).max())
    # without the direct term the rotation block is off by far more than the bound
    r_without = pose_r(T.grad, slab_only, B, E)
    report("normals_pose[normal_map loss]", r=r, rotation_term_share=share, r_without_the_term=r_without)
    print(f"normals_pose: r = {r:.3g}, direct term / total up to {share:.3g}, r without it {r_without:.3g}")
    assert r <= R_MAX, r
    assert r_without > R_MAX          # (the measure can tell: without the term the same gradient misses the bound)


# ---- 5. what it is for -----------------------------------------------------------------------------------------------------
def disc_scene(seed=0, n_side=26):
    """flat discs (log-scales -2.6, -2.6, -6) on the plane through (0, 0, 5) with normal m = (sin 0.35, 0, cos 0.35) of the
    camera frame (identity pose), on a jittered grid, their quaternions turned off the plane's frame by ~0.35 rad"""
    gen = torch.Generator().manual_seed(seed)
    tilt = 0.35
    m = torch.tensor([math.sin(tilt), 0.0, math.cos(tilt)])
    e1 = torch.tensor([math.cos(tilt), 0.0, -math.sin(tilt)])
    e2 = torch.tensor([0.0, 1.0, 0.0])
    u = torch.linspace(-2.2, 2.2, n_side)
    uu, vv = torch.meshgrid(u, u, indexing="ij")
    jitter = 0.03 * torch.randn(n_side * n_side, 2, generator=gen)
    a, b = uu.reshape(-1) + jitter[:, 0], vv.reshape(-1) + jitter[:, 1]
    n = a.numel()
    xyz = torch.tensor([0.0, 0.0, 5.0]) + a[:, None] * e1 + b[:, None] * e2
    # the rotation (e1, e2, m) as a quaternion: a turn by `tilt` about y; then a random small turn on top
    base = torch.tensor([math.cos(tilt / 2), 0.0, math.sin(tilt / 2), 0.0])
    axis = torch.randn(n, 3, generator=gen)
    axis = axis / axis.norm(dim=1, keepdim=True)
    ang = 0.35 * (0.5 + torch.rand(n, generator=gen))
    dq = torch.cat((torch.cos(ang / 2)[:, None], torch.sin(ang / 2)[:, None] * axis), dim=1)
    w1, x1, y1, z1 = base
    w2, x2, y2, z2 = dq.unbind(1)
    q = torch.stack((w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2), dim=1)
    scale = torch.tensor([-2.6, -2.6, -6.0]).repeat(n, 1)
    g = Gaussians(xyz.to(DEV), torch.rand(n, 3, generator=gen).to(DEV), torch.full((n, 1), 2.0, device=DEV),
                  scale.to(DEV), q.to(DEV).contiguous(), None)
    K = torch.tensor([[110.0, 0.0, 64.0], [0.0, 110.0, 64.0], [0.0, 0.0, 1.0]], device=DEV)
    return g, Camera(128, 128, K), torch.eye(4, device=DEV), m


def disc_angle(g, m):
    """the mean angle between the discs' normals (the axis of their smallest scale, up to sign) and the plane's"""
    n, _ = N.gaussian_normals(g.quaternion.detach().cpu(), g.scale.cpu(), torch.eye(4), g.xyz.cpu(), detail=True)
    return float(torch.acos((n @ m.double()).abs().clamp(max=1.0)).mean())


def test_training_on_the_loss_aligns_the_discs():
    g, cam, T, m = disc_scene()
    g.quaternion.requires_grad_(True)
    bg = torch.zeros(3, device=DEV)
    opt = torch.optim.Adam([g.quaternion], lr=0.004)
    marks, losses = (0, 10, 20, 30, 40), {}
    angle0 = disc_angle(g, m)
    for step in range(marks[-1] + 1):
        opt.zero_grad()
        image, depth, alpha, normal_map, mask, uv = fused.rasterize_normals(g, T, cam, **DEFAULTS, use_sh_precompute=True,
                                                                            background_rgb=bg)
        loss = train_ops.normal_consistency_loss(normal_map, depth, alpha, cam)
        if step in marks:
            losses[step] = float(loss.detach())
        if step == marks[-1]:
            break
        loss.backward()
        opt.step()
    angle1 = disc_angle(g, m)
    report("normals_training", angle_before=angle0, angle_after=angle1, **{f"loss_{k}": v for k, v in losses.items()})
    print(f"normals_training: loss {losses}, mean angle {angle0:.4f} -> {angle1:.4f} rad")
    seq = [losses[k] for k in marks]
    assert all(b < a for a, b in zip(seq, seq[1:])), losses
    assert angle1 < angle0, (angle0, angle1)


def test_loss_value_and_all_invalid_frame():
    """the loss on a device frame equals the restatement's on the same maps; an all-invalid frame gives a zero with a graph"""
    m = N.depth_maps(37, 29, False)
    gen = torch.Generator().manual_seed(2)
    nm = torch.randn(29, 37, 3, generator=gen)
    want = N.consistency_loss(nm, m.depth, m.alpha, m.K)
    cam = Camera(37, 29, m.K.to(DEV))
    nm_d = nm.to(DEV).requires_grad_(True)
    got = train_ops.normal_consistency_loss(nm_d, m.depth.to(DEV), m.alpha.to(DEV), cam)
    assert abs(float(got.detach()) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    d = torch.ones(2, 2, device=DEV, requires_grad=True)
    z = train_ops.normal_consistency_loss(torch.ones(2, 2, 3, device=DEV, requires_grad=True), d, torch.ones(2, 2, device=DEV),
                                          Camera(2, 2, m.K.to(DEV)))
    assert float(z.detach()) == 0.0 and z.requires_grad
    z.backward()
    assert d.grad is not None and not d.grad.any()


# ---- 6. the refusals ---------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_and_write_nothing():
    lib, s = _hip.lib(), _hip.current_stream()
    W, H = 20, 18
    depth, alpha = torch.ones(H, W, device=DEV), torch.ones(H, W, device=DEV)
    K = torch.tensor([[20.0, 0.0, 10.0], [0.0, 20.0, 9.0], [0.0, 0.0, 1.0]], device=DEV)
    gn = torch.ones(H, W, 3, device=DEV)
    out = torch.full((H, W, 3), 7.0, device=DEV)
    gd, ga = torch.full((H, W), 7.0, device=DEV), torch.full((H, W), 7.0, device=DEV)
    fwd = lambda **kw: [kw.get("depth", p(depth)), p(alpha), kw.get("K", p(K)), kw.get("W", W), H, kw.get("min_alpha", 0.0),
                        kw.get("mode", 0), kw.get("out", p(out)), s]
    bwd = lambda **kw: [kw.get("depth", p(depth)), p(alpha), kw.get("K", p(K)), kw.get("gn", p(gn)), kw.get("W", W), H,
                        kw.get("min_alpha", 0.0), kw.get("mode", 0), p(gd), kw.get("ga", p(ga)), s]
    cases = ((dict(mode=1), b"raster_mode"), (dict(mode=3), b"raster_mode"), (dict(mode=-1), b"raster_mode"),
             (dict(W=-1), b"negative"), (dict(min_alpha=-0.5), b"min_alpha"), (dict(min_alpha=float("nan")), b"min_alpha"),
             (dict(depth=None), b"NULL"), (dict(K=None), b"NULL"))
    for kw, word in cases:
        assert lib.gs_depth_normal(*fwd(**kw)) == _hip.GS_EINVAL and word in lib.gs_last_error(), kw
        assert lib.gs_depth_normal_backward(*bwd(**kw)) == _hip.GS_EINVAL and word in lib.gs_last_error(), kw
    assert lib.gs_depth_normal(*fwd(out=None)) == _hip.GS_EINVAL and b"NULL" in lib.gs_last_error()
    for kw in (dict(gn=None), dict(ga=None)):
        assert lib.gs_depth_normal_backward(*bwd(**kw)) == _hip.GS_EINVAL and b"NULL" in lib.gs_last_error(), kw
    # an empty image launches nothing
    assert lib.gs_depth_normal(None, None, None, 0, 5, 0.0, 0, None, s) == _hip.GS_OK
    assert lib.gs_depth_normal_backward(None, None, None, None, 5, 0, 0.0, 2, None, None, s) == _hip.GS_OK
    q, sc3, T = torch.ones(4, 4, device=DEV), torch.zeros(4, 3, device=DEV), torch.eye(4, device=DEV)
    pc = torch.ones(4, 3, device=DEV)
    idx = torch.arange(4, dtype=torch.int32, device=DEV)
    nout, gq = torch.full((4, 3), 7.0, device=DEV), torch.full((4, 4), 7.0, device=DEV)
    assert lib.gs_gaussian_normals(p(q), p(sc3), p(T), p(idx), p(pc), -1, p(nout), s) == _hip.GS_EINVAL
    assert b"negative" in lib.gs_last_error()
    for args in ((None, p(sc3), p(T), p(idx), p(pc)), (p(q), p(sc3), p(T), None, p(pc)), (p(q), p(sc3), None, p(idx), p(pc))):
        assert lib.gs_gaussian_normals(*args, 4, p(nout), s) == _hip.GS_EINVAL and b"NULL" in lib.gs_last_error()
    assert lib.gs_gaussian_normals(p(q), p(sc3), p(T), p(idx), p(pc), 4, None, s) == _hip.GS_EINVAL
    assert lib.gs_gaussian_normals(None, None, None, None, None, 0, None, s) == _hip.GS_OK
    back = lambda **kw: [kw.get("q", p(q)), p(sc3), p(T), kw.get("rank", p(idx)), p(pc), kw.get("g", p(nout)), kw.get("V", 4),
                         kw.get("N", 4), kw.get("out", p(gq)), s]
    for kw, word in ((dict(V=-1), b"negative"), (dict(N=-1, V=0), b"negative"), (dict(V=5), b"visible rows"),
                     (dict(q=None), b"NULL"), (dict(rank=None), b"NULL"), (dict(g=None), b"NULL"), (dict(out=None), b"NULL")):
        assert lib.gs_gaussian_normals_backward(*back(**kw)) == _hip.GS_EINVAL and word in lib.gs_last_error(), kw
    assert lib.gs_gaussian_normals_backward(None, None, None, None, None, None, 0, 0, None, s) == _hip.GS_OK
    torch.cuda.synchronize()
    for t in (out, gd, ga, nout, gq):
        assert bool((t == 7.0).all())
    # the package's own checks, on the device
    cam = Camera(W, H, K)
    with pytest.raises(RuntimeError, match="camera_model"):
        fused.depth_to_normal(depth, alpha, cam, camera_model="orthographic")
    with pytest.raises(RuntimeError, match="alpha must match depth"):
        fused.depth_to_normal(depth, alpha[:, :5], cam)
    with pytest.raises(RuntimeError, match="min_alpha"):
        fused.depth_to_normal(depth, alpha, cam, min_alpha=-1.0)
    with pytest.raises(RuntimeError, match="camera.K must be float32"):
        fused.depth_to_normal(depth, alpha, Camera(W, H, K.cpu()))
    g, cam2, T2, bg = frame_inputs(0.0, grads=False)
    args = (g, T2, cam2, DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"], DEFAULTS["mh_dist"])
    for kw, word in ((dict(tile_rows=(0, 2)), "whole single-GPU frames"), (dict(return_aux=True), "whole single-GPU frames"),
                     (dict(adam_plan=object()), "quaternion"), (dict(camera_model="orthographic"), "camera_model")):
        with pytest.raises(RuntimeError, match=word):
            fused.rasterize_normals(*args, True, bg, **kw)
    # and the next frame is served
    out6 = fused.rasterize_normals(*args, True, bg)
    assert len(out6) == 6 and bool(torch.isfinite(out6[3]).all())
