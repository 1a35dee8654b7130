"""The normals of DESIGN.md 7l (include/gsplat_hip.h "Normals") written from their formulas with torch autograd (test code
only): the visible Gaussians' normals, the normal of a rendered depth map, and the normal-consistency loss.  Each takes a
dtype: float64 is the reference, float32 under the same autograd is the error the formulas' own fp32 arithmetic makes --
the envelope of the GPU tests (ref64.r_measure).  Gradients come from autograd; every decision (axis, flip, validity) is
taken without it, so it is a constant there as in the kernels.

  Gaussian normals   qhat = q / |q|, R = quat_to_rot(qhat), a = the index of the smallest log-scale (lowest on a tie),
                     n_c = W R[:, a], negated where n_c . xyz_cam > 0
  depth normals      d = depth / alpha, P = d ray(x, y) at the integer pixel, ray = ((x - cx) / fx, (y - cy) / fy, 1),
                     under the fisheye model (tan(theta) / theta a, 1) with a the same two numbers and theta = |a|
                     (theta == 0: the factor is 1; theta >= pi / 2: no ray).  In float64 the factor is torch.tan's; in
                     float32 it is the kernel's own sequence of +, *, / (tan_over_theta_fp32), which exists so that this
                     file can repeat it -- the fisheye ray then matches the device's to the bit, as the pinhole ray does;
                     n = normalize((P(x, y + 1) - P(x, y - 1)) x (P(x + 1, y) - P(x - 1, y))) where the pixel is off the
                     border, it and its four neighbours have alpha > min_alpha and a ray, and the cross product is not 0
  loss               mean over the valid pixels of alpha - sum_c normal_map_c n_d,c  (alpha a constant)

Fragile elements, named here and left out of the GPU comparisons (tests/test_normals_ref.py caps their share at 0.5 %):
  Gaussian normals   rows with |n_c . xyz_cam / |xyz_cam|| < FLIP_MARGIN in float64: the flip may differ between the
                     precisions.  The axis compares the inputs themselves and is the same in every precision.
  depth normals      pixels whose float64 cross product is shorter than CROSS_MARGIN |D_y P| |D_x P|.  A cross product
                     that is exactly zero (a block of zero depth) is not fragile: it is invalid in every precision."""
import math
from types import SimpleNamespace

import torch

from .ref64 import general_camera_scene

FLIP_MARGIN = 1e-4
CROSS_MARGIN = 1e-6
FRAGILE_CAP = 0.005
N_STAGE = 6000
STAGE_SCENES = {"landscape": 161, "odd": 165}   # kind: seed of general_camera_scene(seed, N_STAGE, kind=kind)
MAP_SIZES = ((37, 29), (16, 16), (33, 17), (50, 1), (1, 50), (2, 2), (517, 301))   # (W, H)


def stage_scene(kind):
    return general_camera_scene(STAGE_SCENES[kind], N_STAGE, kind=kind, stress=True)


def _sqrt(x):
    """the correctly rounded square root in x's dtype (the kernels' is IEEE; torch's float32 one on the CPU is not
    always): through float64, whose square root rounded to float32 is the correctly rounded float32 one"""
    return torch.sqrt(x.double()).to(x.dtype) if x.dtype == torch.float32 else torch.sqrt(x)


# ---- the Gaussians' normals -------------------------------------------------------------------------------------------
def choose_axis(log_scale):
    """[N] int64: the index of the smallest log-scale, the lowest index on a tie; compares the inputs as they are"""
    s = log_scale.detach()
    axis = torch.zeros(s.shape[0], dtype=torch.int64)
    least = s[:, 0].clone()
    one = s[:, 1] < least
    axis[one] = 1
    least = torch.where(one, s[:, 1], least)
    axis[s[:, 2] < least] = 2
    return axis


def gaussian_normals(q, log_scale, T, xyz_cam, dtype=torch.float64, detail=False):
    """normals [V, 3] in dtype of the V Gaussians given (their rows of q, log_scale and of the stage's xyz_camera_frame),
    differentiable in q and T.  detail: -> (normals, SimpleNamespace(axis, flip, n_world, facing)), facing = n_c . p / |p|
    before the flip"""
    axis = choose_axis(log_scale)
    q, T, p = q.to(dtype), T.to(dtype), xyz_cam.detach().to(dtype)
    w, x, y, z = q.unbind(1)
    norm = _sqrt(x * x + y * y + z * z + w * w)
    w, x, y, z = w / norm, x / norm, y / norm, z / norm
    R = torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
                     2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
                     2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y], dim=1).view(-1, 3, 3)
    n_w = R[torch.arange(R.shape[0]), :, axis]
    n_c = n_w @ T[:3, :3].t()
    with torch.no_grad():
        dot = (n_c * p).sum(dim=1)
        flip = dot > 0
    out = torch.where(flip[:, None], -n_c, n_c)
    if not detail:
        return out
    return out, SimpleNamespace(axis=axis, flip=flip, n_world=n_w.detach(),
                                facing=(dot / p.norm(dim=1).clamp(min=1e-300)).detach())


def fragile_rows(q, log_scale, T, xyz_cam):
    """[V] bool: the rows whose flip may differ between float32 and float64"""
    return gaussian_normals(q, log_scale, T, xyz_cam, detail=True)[1].facing.abs() < FLIP_MARGIN


# ---- the depth map's normal --------------------------------------------------------------------------------------------
PIO2_HI, PIO2_LO, PIO4 = float.fromhex("0x1.921fb6p+0"), float.fromhex("-0x1.777a5cp-25"), float.fromhex("0x1.921fb6p-1")
SIN_OVER_X = [float.fromhex(h) for h in ("-0x1.ae6456p-26", "0x1.71de3ap-19", "-0x1.a01a02p-13", "0x1.111112p-7",
                                         "-0x1.555556p-3", "0x1p+0")]
COS = [float.fromhex(h) for h in ("0x1.1eed8ep-29", "-0x1.27e4fcp-22", "0x1.a01a02p-16", "-0x1.6c16c2p-10", "0x1.555556p-5",
                                  "-0x1p-1", "0x1p+0")]


def tan_over_theta_fp32(theta):
    """csrc/normals.hip's tan_over_theta, operation for operation, on a float32 tensor (every constant is a float32 value
    and every torch operation rounds once)"""
    assert theta.dtype == torch.float32
    low = theta <= PIO4
    x = torch.where(low, theta, (PIO2_HI - theta) + PIO2_LO)
    x2 = x * x
    ps = torch.full_like(x2, SIN_OVER_X[0])
    for c in SIN_OVER_X[1:]:
        ps = ps * x2 + c
    pc = torch.full_like(x2, COS[0])
    for c in COS[1:]:
        pc = pc * x2 + c
    safe = torch.where(low, torch.ones_like(theta), theta)
    return torch.where(low, ps / pc, (pc / (x * ps)) / safe)


def rays(K, W, H, fisheye, dtype):
    """-> (ray [H, W, 3], ok [H, W]): the direction whose multiple by d is pixel (x, y)'s back-projection"""
    K = K.detach().to(dtype)
    x = torch.arange(W, dtype=dtype)[None, :].expand(H, W)
    y = torch.arange(H, dtype=dtype)[:, None].expand(H, W)
    rx, ry = (x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1]
    ok = torch.ones(H, W, dtype=torch.bool)
    if fisheye:
        theta = _sqrt(rx * rx + ry * ry)
        if dtype == torch.float32:   # the kernel's own evaluation: the envelope is the error of ITS float32 arithmetic
            ok = theta < PIO2_HI
            s = torch.where(ok, tan_over_theta_fp32(torch.where(ok, theta, torch.zeros_like(theta))), torch.ones_like(theta))
        else:
            ok = theta < math.pi / 2
            safe = torch.where(ok & (theta > 0), theta, torch.ones_like(theta))
            s = torch.where(ok & (theta > 0), torch.tan(safe) / safe, torch.ones_like(theta))
        rx, ry = rx * s, ry * s
    return torch.stack([rx, ry, torch.ones_like(rx)], dim=2), ok


def depth_normal(depth, alpha, K, fisheye=False, min_alpha=0.0, dtype=torch.float64, detail=False):
    """normal [H, W, 3] in dtype, zero where invalid, differentiable in depth and alpha.
    detail: -> (normal, valid [H, W] bool, fragile [H, W] bool)"""
    H, W = depth.shape
    depth, alpha = depth.to(dtype), alpha.to(dtype)
    ray, ray_ok = rays(K, W, H, fisheye, dtype)
    with torch.no_grad():
        has = (alpha > min_alpha) & ray_ok
    d = depth / torch.where(has, alpha, torch.ones_like(alpha))
    P = d[:, :, None] * ray
    normal = torch.zeros(H, W, 3, dtype=dtype)
    valid = torch.zeros(H, W, dtype=torch.bool)
    fragile = torch.zeros(H, W, dtype=torch.bool)
    if H >= 3 and W >= 3:
        a = P[2:, 1:-1] - P[:-2, 1:-1]
        b = P[1:-1, 2:] - P[1:-1, :-2]
        c = torch.linalg.cross(a, b, dim=2)
        n2 = (c * c).sum(dim=2)
        with torch.no_grad():
            all5 = has[1:-1, 1:-1] & has[2:, 1:-1] & has[:-2, 1:-1] & has[1:-1, 2:] & has[1:-1, :-2]
            inner = all5 & (n2 > 0)
            fragile[1:-1, 1:-1] = all5 & (torch.sqrt(n2) < CROSS_MARGIN * a.norm(dim=2) * b.norm(dim=2))
        length = _sqrt(torch.where(inner, n2, torch.ones_like(n2)))
        inner_n = torch.where(inner[:, :, None], c / length[:, :, None], torch.zeros_like(c))
        normal = torch.nn.functional.pad(inner_n, (0, 0, 1, 1, 1, 1))
        valid[1:-1, 1:-1] = inner
    return (normal, valid, fragile) if detail else normal


def consistency_loss(normal_map, depth, alpha, K, fisheye=False, min_alpha=0.0, dtype=torch.float64):
    """mean over the valid pixels of alpha - normal_map . n_d, alpha a constant; a zero with a graph when none is valid"""
    n_d, valid, _ = depth_normal(depth, alpha, K, fisheye, min_alpha, dtype, detail=True)
    per_pixel = alpha.detach().to(dtype) - (normal_map.to(dtype) * n_d).sum(dim=2)
    return torch.where(valid, per_pixel, torch.zeros_like(per_pixel)).sum() / max(int(valid.sum()), 1)


# ---- test maps ---------------------------------------------------------------------------------------------------------
PLANE = (torch.tensor([0.3, -0.2, 0.93]), 4.0)   # m, c of the plane m . P = c in the camera frame


def map_camera(W, H, fisheye):
    """K float32 [3, 3]: a principal point on an integer pixel (the fisheye axis is a pixel of the map: theta == 0), a
    focal length under which the corners of every size stay inside 43 degrees of the axis -- below pi / 4, so these maps
    run the low branch of tan_over_theta only; wide_maps covers the rest"""
    f = 0.9 * max(W, H, 8)
    return torch.tensor([[f, 0.0, float(int(0.45 * W))], [0.0, 1.1 * f, float(int(0.55 * H))], [0.0, 0.0, 1.0]])


def plane_depth(K, W, H, fisheye, m=PLANE[0], c=PLANE[1]):
    """d [H, W] float64: the camera-frame z at which pixel (x, y)'s ray meets the plane m . P = c"""
    ray, ok = rays(K, W, H, fisheye, torch.float64)
    assert bool(ok.all())
    return c / (ray * m.double()).sum(dim=2)


def depth_maps(W, H, fisheye, seed=5, holes=True):
    """-> SimpleNamespace(depth, alpha float32 [H, W] as rasterize_rgbd returns them, K, zero_block, zero_core): a plane plus
    low-frequency sines of amplitude 0.05 (1e5 times fp32's spacing at these depths), alpha in (0.3, 1], with holes a
    rectangle and ~3 % scattered pixels of alpha = 0 and one block of depth = 0 exactly (the degenerate cross product)"""
    gen = torch.Generator().manual_seed(seed + 7 * W + H)
    K = map_camera(W, H, fisheye)
    x = torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    y = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    span = float(max(W, H, 8))
    d = plane_depth(K, W, H, fisheye) + 0.05 * torch.sin(7.0 * x / span + 0.4) * torch.cos(5.0 * y / span - 0.3) \
        + 0.03 * torch.sin(11.0 * (x + y) / span)
    alpha = 0.3 + 0.7 * torch.rand(H, W, generator=gen, dtype=torch.float64).clamp(min=1e-3)
    zero_block = torch.zeros(H, W, dtype=torch.bool)
    if holes:
        alpha[H // 5:H // 5 + max(H // 6, 1), W // 2:W // 2 + max(W // 5, 1)] = 0.0
        alpha[torch.rand(H, W, generator=gen) < 0.03] = 0.0
        zero_block[(3 * H) // 5:(3 * H) // 5 + max(H // 5, 1), W // 8:W // 8 + max(W // 4, 1)] = True
    alpha = alpha.float()
    depth = (d * alpha.double()).float()
    depth[zero_block] = 0.0
    # the block's pixels whose four neighbours lie in it too: both differences are exactly zero there
    core = torch.zeros(H, W, dtype=torch.bool)
    if H >= 3 and W >= 3:
        z = zero_block
        core[1:-1, 1:-1] = z[1:-1, 1:-1] & z[2:, 1:-1] & z[:-2, 1:-1] & z[1:-1, 2:] & z[1:-1, :-2]
    return SimpleNamespace(depth=depth.contiguous(), alpha=alpha.contiguous(), K=K, zero_block=zero_block, zero_core=core,
                           W=W, H=H)


WIDE_SIZES = ((16, 16, 3.0), (61, 47, 21.0))   # (W, H, f): theta from 0 through pi / 4 to beyond pi / 2


def wide_maps(W, H, f, seed=6):
    """-> depth_maps' fields for a short-focal fisheye camera whose rays span the axis, pi / 4 and beyond 90 degrees (the
    corners have no ray), plus ray_ok [H, W] (float64): a bumpy sphere, rho = 4 + low-frequency sines along the ray, so
    d = rho cos(theta) falls to 0 towards 90 degrees; alpha in (0.3, 1] with ~3 % scattered holes.  The principal point
    is off every pixel by a fraction chosen so that no theta lies within 1e-4 of pi / 2"""
    gen = torch.Generator().manual_seed(seed + 7 * W + H)
    K = torch.tensor([[f, 0.0, W / 2 + 0.25], [0.0, 1.1 * f, H / 2 - 0.125], [0.0, 0.0, 1.0]])
    x = torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    y = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    ax, ay = (x - float(K[0, 2])) / float(K[0, 0]), (y - float(K[1, 2])) / float(K[1, 1])
    theta = torch.sqrt(ax * ax + ay * ay)
    assert float((theta - math.pi / 2).abs().min()) > 1e-4
    ok = theta < math.pi / 2
    span = float(max(W, H))
    rho = 4.0 + 0.3 * torch.sin(7.0 * x / span + 0.4) * torch.cos(5.0 * y / span - 0.3) + 0.2 * torch.sin(11.0 * (x + y) / span)
    d = torch.where(ok, rho * torch.cos(theta), torch.ones_like(rho))
    alpha = 0.3 + 0.7 * torch.rand(H, W, generator=gen, dtype=torch.float64).clamp(min=1e-3)
    alpha[torch.rand(H, W, generator=gen) < 0.03] = 0.0
    alpha = alpha.float()
    none = torch.zeros(H, W, dtype=torch.bool)
    return SimpleNamespace(depth=(d * alpha.double()).float().contiguous(), alpha=alpha.contiguous(), K=K, zero_block=none,
                           zero_core=none, W=W, H=H, ray_ok=ok, theta=theta)


def random_normal_grad(H, W, seed):
    """[H, W, 3] float32 whose pixels' magnitudes spread over 1e-4 .. 1 (ref64.random_slab's draw, per pixel)"""
    gen = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (-4.0 * torch.rand(H, W, 1, generator=gen, dtype=torch.float64))
    return (torch.randn(H, W, 3, generator=gen, dtype=torch.float64) * mag).float()
