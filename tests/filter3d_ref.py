"""The 3D smoothing filter (include/gsplat_hip.h "3D smoothing filter") written from its formulas with torch
autograd (test code only), on top of tests/ref64.py and tests/fisheye_ref.py.

  Sigma_eff = R diag(s^2) R^T + phi I          s = exp(log_scale), phi [N] >= 0 a constant
  rho3  = prod_k s_k^2 / (s_k^2 + phi)         comp3 = sqrt(rho3) where rho3 > 0, else 0
  opa3  = sigmoid(logit) comp3                 (antialiased: opa = opa3 comp, comp of tests/antialias_ref.py on the
                                                conic of Sigma_eff)
  d opa3 / d logit   = comp3 y (1 - y)         d opa3 / d log_scale_k = opa3 phi / (s_k^2 + phi)

filtered_stage is ref64.per_gaussian_fp64 with those two changes, in a given dtype: float64 is the reference, float32
under the same autograd is the error the formulas' own fp32 arithmetic makes -- the envelope of the GPU tests.  With
camera_T_world [4, 4] it uses per_gaussian_fp64's expressions in their order (so phi = 0 in float64 returns its values
exactly); with one pose per Gaussian [N, 4, 4] the gradient of the poses is the list of per-Gaussian terms of
camera_T_world's gradient (tests/pose_terms.py's t64 / t32).

comp of 7e cancels (det_0 = a0 c0 - b b), so its fp32 value depends on the last bits of the conic it is given: as in
tests/test_gpu_antialias.py, whose envelope evaluates the factor on the conic the kernels computed, filtered_stage takes
conic_bits = (rows, conic of those rows) and evaluates the 2D factor -- value and derivative -- at those bits, the rest of
the chain staying its own.

rate_of is the sampling rate over a list of cameras, from_rate the filter made of it."""
import functools
from types import SimpleNamespace

import torch

from . import fisheye_ref
from .ref64 import (_f32, LEAVES, R_SH_0, camera_center, general_camera_scene, look_at_pose, quat_to_rot, sh_basis)

N_STAGE = 6000
SCENES = (("landscape", 3), ("portrait", 1), ("odd", 0))     # general_camera_scene(150 + deg, N_STAGE, deg, kind) + tiny rows
# (antialiased, fisheye): the three modes of the issue, and the fisheye model without the 2D factor (its own instantiations)
MODES = {"filter": (False, False), "filter+aa": (True, False), "filter+aa+fisheye": (True, True),
         "filter+fisheye": (False, True)}
CAMERA_COUNTS = (1, 5, 67)
EDGE_PX, NEAR_REL = 1e-3, 1e-6


def aa_comp(conic):
    """comp [V] of tests/antialias_ref.py in conic's dtype, differentiable"""
    s00, s01, s11 = conic[:, 0], conic[:, 1] / 2, conic[:, 2]
    det_0 = s00 * s11 - s01 * s01
    det_d = (s00 + 0.25) * (s11 + 0.25) - s01 * s01
    with torch.no_grad():
        ok = (det_0 > 0) & (det_d > 0)
    rho = torch.where(ok, det_0 / torch.where(ok, det_d, torch.ones_like(det_d)), torch.ones_like(det_0))
    return torch.where(ok, torch.sqrt(rho), torch.zeros_like(rho)), det_0


def comp3_of(log_scale, phi):
    """comp3 [N] in log_scale's dtype, differentiable in log_scale; phi [N]"""
    s2 = torch.exp(log_scale) ** 2
    # (phi == 0: the quotient is the constant 1; kept out of autograd, whose 1 / s^4 leaves fp32's range for the rows of
    # log-scale -50)
    pos = (phi > 0)[:, None].expand_as(s2)
    quot = torch.where(pos, s2 / torch.where(pos, s2 + phi[:, None], torch.ones_like(s2)), torch.ones_like(s2))
    rho3 = quot[:, 0] * quot[:, 1] * quot[:, 2]
    with torch.no_grad():
        ok = rho3 > 0
    return torch.where(ok, torch.sqrt(torch.where(ok, rho3, torch.ones_like(rho3))), torch.zeros_like(rho3))


def closed_form_terms(log_scale, logit, phi, g):
    """the header's backward of opa3: g [N] = dL/d opa3 -> (grad_opacity_logit [N], the scale gradient's term [N, 3]),
    in the inputs' dtype; comp3 == 0 rows get zeros"""
    s2 = torch.exp(log_scale) ** 2
    comp3 = comp3_of(log_scale, phi)
    y = torch.sigmoid(logit.reshape(-1))
    pos = comp3 > 0
    go = torch.where(pos, g * comp3 * (1 - y) * y, torch.zeros_like(g))
    gs = torch.where(pos[:, None], (g * (y * comp3) * phi)[:, None] / (s2 + phi[:, None]), torch.zeros_like(s2))
    return go, gs


def filtered_stage(xyz, q, log_scale, opacity_logit, rgb, sh, phi, T, K, width, height, near, far, pad,
                   dtype=torch.float64, antialiased=False, fisheye=False, conic_bits=None):
    """the per-Gaussian stage with the filter phi [N] (None: without it), evaluated in `dtype` (the parameter tensors
    are passed in that dtype).  T: [4, 4], or [N, 4, 4] one pose per Gaussian.  -> dict uv, xyz_cam, conic, opacity_act
    (the sigmoid), opa (what the record's opacity column holds), comp3, det_0 (of the conic), rgb_render, packed_abc,
    culled."""
    T, K = T.to(dtype), K.to(dtype)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    per_row = T.dim() == 3
    if per_row:
        A, t = T[:, :3, :3], T[:, :3, 3]
        c = (A @ xyz[:, :, None])[:, :, 0] + t
    else:
        A, t = T[:3, :3], T[:3, 3]
        c = xyz @ A.T + t
    x, y, z = c.unbind(1)
    if fisheye:
        uv = fisheye_ref.project(c, fx, fy, cx, cy)
        J = fisheye_ref.jacobian(c, fx, fy)
    else:
        uv = torch.stack([fx * x / z + cx, fy * y / z + cy], dim=1)
        zero = torch.zeros_like(z)
        J = torch.stack([fx / z, zero, -fx * x / (z * z), zero, fy / z, -fy * y / (z * z)], dim=1).view(-1, 2, 3)
    with torch.no_grad():
        u, v = uv.unbind(1)
        culled = ((z < _f32(near)) | (z > _f32(far)) | (u < _f32(-pad)) | (u > _f32(width + pad)) |
                  (v < _f32(-pad)) | (v > _f32(height + pad)))
    R = quat_to_rot(q)
    M = R * torch.exp(log_scale)[:, None, :]
    sigma = M @ M.transpose(1, 2)
    if phi is not None:
        sigma = sigma + phi.to(dtype)[:, None, None] * torch.eye(3, dtype=dtype)
    JA = J @ A
    s2 = JA @ sigma @ JA.transpose(1, 2)
    conic = torch.stack([s2[:, 0, 0], s2[:, 0, 1] + s2[:, 1, 0], s2[:, 1, 1]], dim=1)
    opacity_act = torch.sigmoid(opacity_logit)
    comp3 = comp3_of(log_scale, phi.to(dtype)) if phi is not None else torch.ones_like(z)
    opa = opacity_act * comp3[:, None] if phi is not None else opacity_act
    conic_aa = conic
    if conic_bits is not None:
        rows, bits = conic_bits
        shift = torch.zeros_like(conic)
        shift[rows] = (bits.to(dtype) - conic[rows]).detach()
        conic_aa = conic + shift     # (exact: the two values are within a factor of two of each other, or the row is far off)
    comp, det_0 = aa_comp(conic_aa)
    if antialiased:
        opa = opa * comp[:, None]
    if sh is None:
        colour = rgb
    else:
        with torch.no_grad():
            centre = camera_center(T if not per_row else T[0]).to(dtype)
            d = xyz - centre
            d = d / d.norm(dim=1, keepdim=True)
            Y = sh_basis(d, sh.shape[2] + 1)
        coeff = torch.cat([rgb.unsqueeze(2), sh], dim=2)
        colour = R_SH_0 * (coeff * Y[:, None, :]).sum(dim=2)
    abc = torch.stack([conic[:, 0] + 0.25, conic[:, 1] / 2, conic[:, 2] + 0.25], dim=1)
    return dict(uv=uv, xyz_cam=c, conic=conic, opacity_act=opacity_act, opa=opa, comp3=comp3, det_0=det_0,
                rgb_render=colour, packed_abc=abc, culled=culled)


def stage(sc, phi, dtype, mode="filter", slab=None, rows=None, pose_terms=False, conic_bits=None):
    """filtered_stage on scene sc in `dtype` under MODES[mode].  slab [len(rows), 9] (rows: Gaussian indices) -> also
    "grad": the dense vector-Jacobian product of the slab with (rgb | opa | uv | conic) of those rows, keyed like LEAVES;
    pose_terms: and "pose_terms" [len(rows), 3, 4], each row's term of camera_T_world's gradient (dL/dA | dL/dt)"""
    aa, fish = MODES[mode]
    L = fisheye_ref.leaves(sc.g, dtype, requires_grad=slab is not None and not pose_terms)
    T = sc.T.to(dtype)
    if pose_terms:
        T = T[None].repeat(sc.g.xyz.shape[0], 1, 1).requires_grad_(True)
    out = filtered_stage(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"],
                         None if phi is None else phi.to(dtype), T, sc.cam.K, sc.W, sc.H, sc.near, sc.far, sc.pad, dtype,
                         aa, fish, conic_bits)
    if slab is not None:
        rows = torch.as_tensor(rows, dtype=torch.long)
        y = torch.cat([out["rgb_render"][rows], out["opa"][rows], out["uv"][rows], out["conic"][rows]], dim=1)
        if pose_terms:
            (gT,) = torch.autograd.grad(y, T, grad_outputs=slab.to(dtype))
            out["pose_terms"] = gT[rows, :3, :]
        else:
            keys = [k for k in LEAVES if L[k] is not None]
            grads = torch.autograd.grad(y, [L[k] for k in keys], grad_outputs=slab.to(dtype), allow_unused=True)
            out["grad"] = {k: (torch.zeros_like(L[k]) if gr is None else gr) for k, gr in zip(keys, grads)}
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


# ---- the rate ------------------------------------------------------------------------------------------------------------
def rate_of(xyz, Ts, Ks, sizes, near=0.2, pad=0.15, dtype=torch.float64, fisheye=False, rate=None, detail=False):
    """max over the cameras that see a Gaussian of max(fx, fy) / depth (depth: z, fisheye |xyz_cam|), starting from `rate`
    (zeros by default), in `dtype`.  Ts [C, 4, 4], Ks [C, 3, 3], sizes [C, 2] = (W, H).  near and pad are compared as the
    fp32 values the kernel receives.  detail: -> (rate, seen [C, N] bool, fragile [N] bool: a row within EDGE_PX of a
    padded image edge or NEAR_REL (relative) of near in some camera)"""
    xyz = xyz.detach().cpu().to(dtype)
    N = xyz.shape[0]
    out = torch.zeros(N, dtype=dtype) if rate is None else rate.detach().cpu().to(dtype).clone()
    seen_all, fragile = [], torch.zeros(N, dtype=torch.bool)
    near, pad = _f32(near), _f32(pad)
    for k in range(Ts.shape[0]):
        T, K = Ts[k].cpu().to(dtype), Ks[k].cpu().to(dtype)
        W, H = float(sizes[k][0]), float(sizes[k][1])
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        c = xyz @ T[:3, :3].T + T[:3, 3]
        z = c[:, 2]
        if fisheye:
            uv = fisheye_ref.project(c, fx, fy, cx, cy)
            depth = c.norm(dim=1)
        else:
            uv = torch.stack([fx * c[:, 0] / z + cx, fy * c[:, 1] / z + cy], dim=1)
            depth = z
        u, v = uv.unbind(1)
        edges = ((u, -pad * W), (u, W + pad * W), (v, -pad * H), (v, H + pad * H))
        seen = (z > near) & (u > edges[0][1]) & (u < edges[1][1]) & (v > edges[2][1]) & (v < edges[3][1])
        r = torch.maximum(fx, fy) / depth
        out = torch.where(seen & (r > out), r, out)
        seen_all.append(seen)
        if detail:
            for val, edge in edges:
                fragile |= (val - edge).abs() < EDGE_PX
            fragile |= (z - near).abs() < NEAR_REL * near
    return (out, torch.stack(seen_all), fragile) if detail else out


def from_rate(rate, variance=0.2):
    """phi = variance / rate^2; rows with rate == 0 take the largest phi of the others; zeros when every rate is 0"""
    seen = rate > 0
    if not bool(seen.any()):
        return torch.zeros_like(rate)
    phi = variance / (torch.where(seen, rate, torch.ones_like(rate)) ** 2)
    return torch.where(seen, phi, phi[seen].max())


# ---- the scenes ------------------------------------------------------------------------------------------------------------
def phi_of(sc, seed):
    """the filter of a stage scene: 3 % of the rows exactly 0, 3 % at 1e6 times the row's largest s^2, the rest
    10^U(-8, 0) times it (float32)"""
    gen = torch.Generator().manual_seed(seed)
    N = sc.g.xyz.shape[0]
    s2max = (torch.exp(sc.g.scale.double()) ** 2).max(dim=1).values
    pick = torch.rand(N, generator=gen, dtype=torch.float64)
    factor = 10.0 ** (-8.0 * torch.rand(N, generator=gen, dtype=torch.float64))
    factor = torch.where(pick < 0.03, torch.zeros_like(factor), factor)
    factor = torch.where(pick > 0.97, torch.full_like(factor, 1e6), factor)
    return (factor * s2max).float().contiguous()


@functools.lru_cache(maxsize=None)
def scene(kind):
    """the stage scene of `kind` with the eight tiny rows of tests/test_gpu_antialias.py and its filter (sc.phi)"""
    from .test_gpu_antialias import with_tiny_rows
    deg = dict(SCENES)[kind]
    sc = with_tiny_rows(general_camera_scene(150 + deg, N_STAGE, deg=deg, kind=kind))
    sc.phi = phi_of(sc, 7 + deg)
    return sc


@functools.lru_cache(maxsize=None)
def camera_set(kind, C):
    """the scene's own camera and C - 1 more looking at the cluster's mean from distances 4 .. 16, every other one with
    the image transposed -> SimpleNamespace(Ts [C,4,4], Ks [C,3,3], sizes [C,2] int32), float32"""
    sc = scene(kind)
    gen = torch.Generator().manual_seed(1000 + C)
    target = sc.g.xyz.double().mean(dim=0)
    Ts, Ks, sizes = [sc.T.double()], [sc.cam.K.double()], [(sc.W, sc.H)]
    for k in range(1, C):
        dist = 4.0 + 12.0 * float(torch.rand(1, generator=gen, dtype=torch.float64))
        A, centre = look_at_pose(gen, target, dist)
        T = torch.eye(4, dtype=torch.float64)
        T[:3, :3], T[:3, 3] = A, -A @ centre
        K = sc.cam.K.double().clone()
        W, H = (sc.W, sc.H) if k % 2 == 0 else (sc.H, sc.W)
        if k % 2:
            K[0, 2], K[1, 2] = K[1, 2].clone(), K[0, 2].clone()
        Ts.append(T)
        Ks.append(K)
        sizes.append((W, H))
    return SimpleNamespace(Ts=torch.stack(Ts).float().contiguous(), Ks=torch.stack(Ks).float().contiguous(),
                           sizes=torch.tensor(sizes, dtype=torch.int32))
