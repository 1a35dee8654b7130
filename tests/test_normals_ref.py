"""tests/normals_ref.py held to what the GPU tests need from it, on the CPU: known answers (a plane seen by a pinhole and
by a fisheye camera, a flat Gaussian in front of an identity camera, ties), gradcheck of both restatements in float64,
the loss of a consistent frame, and the caps on the fragile elements of every scene and map the GPU tests use."""
import math

import pytest
import torch

from . import normals_ref as N

EYE = torch.eye(4)


@pytest.mark.parametrize("fisheye", [False, True])
@pytest.mark.parametrize("W,H", [(37, 29), (16, 16), (64, 48)])
def test_plane_known_answer(W, H, fisheye):
    """the plane m . P = c (c > 0, in front of the camera): the depth normal is -m / |m| at every valid pixel"""
    K = N.map_camera(W, H, fisheye)
    d = N.plane_depth(K, W, H, fisheye)
    alpha = 0.5 + 0.5 * torch.rand(H, W, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    n, valid, fragile = N.depth_normal(d * alpha, alpha, K, fisheye, detail=True)
    m = N.PLANE[0].double()
    assert int(valid.sum()) == (W - 2) * (H - 2) and not fragile.any()
    assert float((n[valid] + m / m.norm()).abs().max()) <= 1e-12
    assert not n[~valid].any()
    if fisheye:   # the axis is a pixel of the map: theta == 0 there
        assert float(K[0, 2]) == int(K[0, 2]) and float(K[1, 2]) == int(K[1, 2])


def test_fisheye_rays_beyond_ninety_degrees_are_invalid():
    K = torch.tensor([[3.0, 0.0, 8.0], [0.0, 3.0, 8.0], [0.0, 0.0, 1.0]])
    ray, ok = N.rays(K, 16, 16, True, torch.float64)
    x = torch.arange(16.0)
    theta = torch.sqrt(((x[None, :] - 8) / 3) ** 2 + ((x[:, None] - 8) / 3) ** 2)
    assert torch.equal(ok, theta.double() < math.pi / 2) and bool(ok.any()) and not bool(ok.all())
    n, valid, _ = N.depth_normal(torch.ones(16, 16), torch.ones(16, 16), K, True, detail=True)
    assert not valid[~ok].any() and bool(valid.any()) and not n[~valid].any()


def test_flat_gaussian_faces_the_camera():
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    s = torch.tensor([[0.0, 0.0, -3.0]])
    p = torch.tensor([[0.2, -0.1, 5.0]])
    n, info = N.gaussian_normals(q, s, EYE, p, detail=True)
    assert torch.equal(n, torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64))
    assert int(info.axis[0]) == 2 and bool(info.flip[0])
    # behind the plane of the disc: not flipped; exactly on it (n . p == 0): not flipped either
    n = N.gaussian_normals(q, s, EYE, torch.tensor([[0.0, 0.0, -5.0]]))
    assert torch.equal(n, torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64))
    n = N.gaussian_normals(q, s, EYE, torch.tensor([[1.0, 1.0, 0.0]]))
    assert torch.equal(n, torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64))
    # the quaternion's length does not matter
    n = N.gaussian_normals(37.0 * q, s, EYE, p)
    assert torch.equal(n, torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64))


def test_ties_take_the_lowest_index():
    s = torch.tensor([[-1.0, -1.0, -1.0], [0.0, -2.0, -2.0], [-2.0, 0.0, -2.0], [-2.0, -2.0, 0.0], [0.0, 0.0, -1.0],
                      [0.5, -0.5, 0.0]])
    assert N.choose_axis(s).tolist() == [0, 1, 0, 0, 2, 1]


def test_gradcheck_gaussian_normals():
    gen = torch.Generator().manual_seed(3)
    q = torch.randn(7, 4, generator=gen, dtype=torch.float64, requires_grad=True)
    s = torch.randn(7, 3, generator=gen, dtype=torch.float64)
    A = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))[0]
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = A
    T.requires_grad_(True)
    p = torch.randn(7, 3, generator=gen, dtype=torch.float64)
    assert float(N.gaussian_normals(q, s, T, p, detail=True)[1].facing.abs().min()) > 1e-3
    assert torch.autograd.gradcheck(lambda q_, T_: N.gaussian_normals(q_, s, T_, p), (q, T))


@pytest.mark.parametrize("fisheye", [False, True])
def test_gradcheck_depth_normal(fisheye):
    m = N.depth_maps(9, 8, fisheye, holes=False)
    depth = m.depth.double().requires_grad_(True)
    alpha = m.alpha.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda d_, a_: N.depth_normal(d_, a_, m.K, fisheye), (depth, alpha))
    # with holes and a threshold: the validity is a constant
    m = N.depth_maps(9, 8, fisheye)
    depth = m.depth.double().requires_grad_(True)
    alpha = m.alpha.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda d_, a_: N.depth_normal(d_, a_, m.K, fisheye, 0.35), (depth, alpha))


@pytest.mark.parametrize("fisheye", [False, True])
def test_loss_of_a_consistent_frame_is_zero(fisheye):
    m = N.depth_maps(37, 29, fisheye)
    n_d, valid, _ = N.depth_normal(m.depth, m.alpha, m.K, fisheye, detail=True)
    assert 0 < int(valid.sum()) < 37 * 29
    loss = N.consistency_loss(m.alpha.double()[:, :, None] * n_d, m.depth, m.alpha, m.K, fisheye)
    assert abs(float(loss)) <= 1e-15
    # normals turned away: alpha - (-alpha) = 2 alpha on average over the valid pixels
    loss = N.consistency_loss(-m.alpha.double()[:, :, None] * n_d, m.depth, m.alpha, m.K, fisheye)
    assert abs(float(loss) - 2 * float(m.alpha.double()[valid].mean())) <= 1e-12
    # nothing valid: a zero that still carries the graph
    nm = torch.ones(2, 2, 3, dtype=torch.float64, requires_grad=True)
    loss = N.consistency_loss(nm, torch.ones(2, 2), torch.ones(2, 2), m.K, fisheye)
    assert float(loss.detach()) == 0.0 and loss.requires_grad


@pytest.mark.parametrize("kind", list(N.STAGE_SCENES))
def test_cap_on_fragile_gaussian_rows(kind):
    sc = N.stage_scene(kind)
    T = sc.T
    p = sc.g.xyz @ T[:3, :3].t() + T[:3, 3]
    fragile = N.fragile_rows(sc.g.quaternion, sc.g.scale, T, p)
    share = float(fragile.float().mean())
    print(f"normals_ref[{kind}]: {int(fragile.sum())} of {fragile.numel()} rows within {N.FLIP_MARGIN} of the flip")
    assert share <= N.FRAGILE_CAP, share
    # float32 and float64 agree on every decision elsewhere
    _, i64 = N.gaussian_normals(sc.g.quaternion, sc.g.scale, T, p, detail=True)
    _, i32 = N.gaussian_normals(sc.g.quaternion, sc.g.scale, T, p, torch.float32, detail=True)
    assert torch.equal(i64.axis, i32.axis) and torch.equal(i64.flip[~fragile], i32.flip[~fragile])
    assert len(set(i64.axis.tolist())) == 3


@pytest.mark.parametrize("fisheye", [False, True])
@pytest.mark.parametrize("W,H", N.MAP_SIZES)
def test_cap_on_fragile_pixels(W, H, fisheye):
    m = N.depth_maps(W, H, fisheye)
    n64, v64, fragile = N.depth_normal(m.depth, m.alpha, m.K, fisheye, detail=True)
    n32, v32, _ = N.depth_normal(m.depth, m.alpha, m.K, fisheye, dtype=torch.float32, detail=True)
    share = float(fragile.float().mean())
    assert share <= N.FRAGILE_CAP, share
    assert torch.equal(v64[~fragile], v32[~fragile])
    assert not v64[m.zero_core].any() and not v32[m.zero_core].any()   # the degenerate pixels: invalid in both
    if min(W, H) < 3:
        assert not v64.any()
    elif W * H > 256:
        assert 0.3 < float(v64.float().mean()) < 1.0 and bool((m.alpha == 0).any()) and bool(m.zero_core.any())
        assert float((n32.double() - n64)[v64].abs().max()) < 1e-2


TAN_BOUND = 4 * 2.0 ** -23


def test_tan_over_theta_fp32_against_float64():
    """the kernel's tan(theta) / theta, as this file repeats it, against float64 over [0, pi / 2): at most eight roundings
    of half an ulp each reach the result (the last Horner step of either series, their quotient; beyond pi / 4 the sum
    that forms x, x times the sine series, two quotients), 4 * 2^-23 = 4.8e-7 relative; measured 2.6e-7 at worst.  Both
    branches, the axis, the threshold and the last float below pi / 2"""
    gen = torch.Generator().manual_seed(0)
    theta = torch.cat([torch.rand(1_000_000, generator=gen, dtype=torch.float64) * (math.pi / 2),
                       torch.linspace(0.0, math.pi / 2, 200_001, dtype=torch.float64)[:-1],
                       torch.tensor([0.0, N.PIO4, 0.785398, 0.7853983, 1.5, 1.57, 1.5707, 1.570796, 1.5707962])]).float()
    theta = theta[theta < N.PIO2_HI]
    got = N.tan_over_theta_fp32(theta).double()
    t64 = theta.double()
    want = torch.where(t64 > 0, torch.tan(t64) / t64.clamp(min=1e-300), torch.ones_like(t64))
    rel = (got - want).abs() / want
    worst = int(rel.argmax())
    print(f"tan_over_theta_fp32: worst relative error {float(rel[worst]):.3g} at theta {float(theta[worst]):.6f}")
    assert bool(torch.isfinite(got).all()) and float(rel.max()) <= TAN_BOUND, (float(rel.max()), float(theta[worst]))
    assert float(got[theta == 0][0]) == 1.0
    assert bool((theta > N.PIO4).any()) and bool((theta <= N.PIO4).any())
    # a wrong constant does not pass: the sine series' x^2 coefficient off by one part in 1e5
    saved = N.SIN_OVER_X[4]
    try:
        N.SIN_OVER_X[4] = saved * (1 + 1e-5)
        bad = N.tan_over_theta_fp32(theta).double()
    finally:
        N.SIN_OVER_X[4] = saved
    assert float(((bad - want).abs() / want).max()) > TAN_BOUND


@pytest.mark.parametrize("W,H,f", N.WIDE_SIZES)
def test_cap_on_fragile_pixels_of_the_wide_maps(W, H, f):
    """the short-focal fisheye maps of the GPU test: rays on both sides of pi / 4 and of pi / 2, the same validity in both
    precisions outside the fragile pixels, which stay under the cap; no valid pixel has a neighbour without a ray"""
    m = N.wide_maps(W, H, f)
    assert float(m.theta.min()) < N.PIO4 < float(m.theta[m.ray_ok].max()) and not bool(m.ray_ok.all())
    assert int((m.ray_ok & (m.theta > N.PIO4)).sum()) > 20
    n64, v64, fragile = N.depth_normal(m.depth, m.alpha, m.K, True, detail=True)
    n32, v32, _ = N.depth_normal(m.depth, m.alpha, m.K, True, dtype=torch.float32, detail=True)
    ray32_ok = N.rays(m.K, W, H, True, torch.float32)[1]
    assert torch.equal(ray32_ok, m.ray_ok)
    assert float(fragile.float().mean()) <= N.FRAGILE_CAP
    assert torch.equal(v64[~fragile], v32[~fragile]) and bool(v64.any())
    no_ray = ~m.ray_ok
    near_no_ray = no_ray.clone()
    near_no_ray[1:] |= no_ray[:-1]
    near_no_ray[:-1] |= no_ray[1:]
    near_no_ray[:, 1:] |= no_ray[:, :-1]
    near_no_ray[:, :-1] |= no_ray[:, 1:]
    assert not v64[near_no_ray].any() and not v32[near_no_ray].any() and not n64[near_no_ray].any()
    assert int((v64 & (m.theta > N.PIO4)).sum()) > 10          # valid pixels beyond the threshold between the branches
