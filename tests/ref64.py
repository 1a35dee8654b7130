"""A plain float64 reference of the per-Gaussian stage, scenes seen through general cameras, and the oracle's
per-stage kernels chained in either precision (test code only).

per_gaussian_fp64 is written from the formulas with torch autograd, not from the kernels:

  xyz_cam = A p + t                        (A, t: the rotation block and translation of camera_T_world)
  uv      = (fx x / z + cx, fy y / z + cy)
  culled  = z < near | z > far | u < -pad | u > W + pad | v < -pad | v > H + pad
  Sigma   = R S S^T R^T,  R from the normalised quaternion (w, x, y, z), S = diag(exp(log_scale))
  J       = [[fx / z, 0, -fx x / z^2], [0, fy / z, -fy y / z^2]]
  Sigma2D = J A Sigma A^T J^T,  conic = (Sigma2D_00, Sigma2D_01 + Sigma2D_10, Sigma2D_11)
  opacity = sigmoid(logit)
  colour  = rgb (degree 0), or r_SH_0 * sum_s Y_s(d) coeff_s with coeff_0 = rgb, coeff_1.. = sh, and d the
            normalised direction from the camera centre -A^-1 t to p

The view direction carries no gradient (the reference's SH backward returns the coefficients' gradient only).
The SH constants are the project's fp32 literals (the kernels and the oracle share them; the exact values differ by
~3e-8 relative, which would hide inside the fp32 envelope but not inside the 1e-10 agreement with the fp64 oracle).
The frustum thresholds are compared as the fp32 values the kernels receive."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from gaussian_splatting_amd.splat_py.structs import Camera, Gaussians

from . import helpers


def _f32(x):
    return float(np.float32(x))


SH_0 = _f32(0.28209479177387814)
R_SH_0 = _f32(3.544907701811032)
SH_1 = _f32(0.4886025119029199)
SH_2 = (_f32(1.0925484305920792), _f32(0.31539156525252005), _f32(0.5462742152960396))
SH_3 = (_f32(0.5900435899266435), _f32(2.890611442640554), _f32(0.4570457994644658), _f32(0.263875515352797),
        _f32(1.445305721320277))
SLAB_WIDTH = 9   # rgb 3 | opacity 1 | uv 2 | conic 3: the layout gs_preprocess_backward takes
LEAVES = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")


def sh_basis(d, n_sh):
    """[N, n_sh] real SH basis at unit directions d [N, 3] (degree 0-3, the project's sign convention)"""
    x, y, z = d.unbind(1)
    Y = [torch.full_like(x, SH_0)]
    if n_sh >= 4:
        Y += [-SH_1 * y, SH_1 * z, -SH_1 * x]
    if n_sh >= 9:
        c0, c2, c4 = SH_2
        Y += [c0 * x * y, -c0 * y * z, c2 * (3 * z * z - 1), -c0 * x * z, c4 * (x * x - y * y)]
    if n_sh >= 16:
        k0, k1, k2, k3, k5 = SH_3
        Y += [-k0 * y * (3 * x * x - y * y), k1 * x * y * z, -k2 * y * (5 * z * z - 1), k3 * z * (5 * z * z - 3),
              -k2 * x * (5 * z * z - 1), k5 * z * (x * x - y * y), -k0 * x * (x * x - 3 * y * y)]
    return torch.stack(Y, dim=1)


def quat_to_rot(q):
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


def camera_center(T):
    T = T.double()
    return -torch.linalg.solve(T[:3, :3], T[:3, 3])


def per_gaussian_fp64(xyz, q, log_scale, opacity_logit, rgb, sh, T, K, width, height, near, far, pad, view_xyz=None):
    """The per-Gaussian stage of every Gaussian in float64 (differentiable in the six parameter tensors, which the
    caller passes as float64; view_xyz: the positions the SH view directions are taken from, xyz by default).  -> dict uv, xyz_cam, conic, opacity_act [N,1], rgb_render, packed_abc (the render
    record's a = conic0 + 1/4, b = conic1 / 2, c = conic2 + 1/4) and culled [N] bool."""
    T, K = T.double(), K.double()
    A, t = T[:3, :3], T[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    c = xyz @ A.T + t
    x, y, z = c.unbind(1)
    uv = torch.stack([fx * x / z + cx, fy * y / z + cy], dim=1)
    with torch.no_grad():
        u, v = uv.unbind(1)
        culled = ((z < _f32(near)) | (z > _f32(far)) | (u < _f32(-pad)) | (u > _f32(width + pad)) |
                  (v < _f32(-pad)) | (v > _f32(height + pad)))
    R = quat_to_rot(q)
    M = R * torch.exp(log_scale)[:, None, :]            # R S
    sigma = M @ M.transpose(1, 2)
    zero = torch.zeros_like(z)
    J = torch.stack([fx / z, zero, -fx * x / (z * z), zero, fy / z, -fy * y / (z * z)], dim=1).view(-1, 2, 3)
    JA = J @ A
    s2 = JA @ sigma @ JA.transpose(1, 2)
    conic = torch.stack([s2[:, 0, 0], s2[:, 0, 1] + s2[:, 1, 0], s2[:, 1, 1]], dim=1)
    opacity_act = torch.sigmoid(opacity_logit)
    if sh is None:
        colour = rgb
    else:
        n_sh = sh.shape[2] + 1
        with torch.no_grad():
            d = (xyz if view_xyz is None else view_xyz) - camera_center(T)
            d = d / d.norm(dim=1, keepdim=True)
            Y = sh_basis(d, n_sh)
        coeff = torch.cat([rgb.unsqueeze(2), sh], dim=2)  # [N, 3, n_sh]
        colour = R_SH_0 * (coeff * Y[:, None, :]).sum(dim=2)
    abc = torch.stack([conic[:, 0] + 0.25, conic[:, 1] / 2, conic[:, 2] + 0.25], dim=1)
    return dict(uv=uv, xyz_cam=c, conic=conic, opacity_act=opacity_act, rgb_render=colour, packed_abc=abc,
                culled=culled)


def leaves64(g, requires_grad=True):
    """float64 leaf copies of the six parameter tensors of Gaussians g (CPU)"""
    out = {}
    for k in LEAVES:
        v = getattr(g, k)
        out[k] = None if v is None else v.detach().cpu().double().clone().requires_grad_(requires_grad)
    return out


def ref64_stage(sc, slab=None, rows=None):
    """ref64 on scene sc.  slab [len(rows), 9] (rows: Gaussian indices) -> also the dense float64 vector-Jacobian
    product of the slab with (rgb | opacity | uv | conic) of those rows, keyed like LEAVES."""
    L = leaves64(sc.g, requires_grad=slab is not None)
    out = per_gaussian_fp64(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], sc.T, sc.cam.K,
                            sc.W, sc.H, sc.near, sc.far, sc.pad)
    if slab is not None:
        rows = torch.as_tensor(rows, dtype=torch.long)
        y = torch.cat([out["rgb_render"][rows], out["opacity_act"][rows], out["uv"][rows], out["conic"][rows]], dim=1)
        keys = [k for k in LEAVES if L[k] is not None]
        grads = torch.autograd.grad(y, [L[k] for k in keys], grad_outputs=slab.double(), allow_unused=True)
        out["grad"] = {k: (torch.zeros_like(L[k]) if gr is None else gr) for k, gr in zip(keys, grads)}
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


def ref64_abs_vjp(sc, a_slab, rows):
    """sum over the nine slab columns j of |d y_j / d leaf| * a_j for Gaussians `rows` (a_slab [len(rows), 9] >= 0), in
    float64: how far a render-gradient error of at most a_j per slab element can move each leaf gradient.  (Each leaf
    row depends on its own Gaussian's outputs only, so one VJP per column gives every term on its own.)"""
    L = leaves64(sc.g)
    out = per_gaussian_fp64(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], sc.T, sc.cam.K,
                            sc.W, sc.H, sc.near, sc.far, sc.pad)
    rows = torch.as_tensor(rows, dtype=torch.long)
    y = torch.cat([out["rgb_render"][rows], out["opacity_act"][rows], out["uv"][rows], out["conic"][rows]], dim=1)
    keys = [k for k in LEAVES if L[k] is not None]
    acc = {k: torch.zeros_like(L[k]) for k in keys}
    a_slab = a_slab.double()
    for j in range(SLAB_WIDTH):
        go = torch.zeros_like(y)
        go[:, j] = a_slab[:, j]
        grads = torch.autograd.grad(y, [L[k] for k in keys], grad_outputs=go, retain_graph=True, allow_unused=True)
        for k, gr in zip(keys, grads):
            if gr is not None:
                acc[k] += gr.detach().abs()
    return acc


# ---- the oracle's per-stage kernels chained (tests/helpers.py) on a scene of general_camera_scene --------------------
def oracle_stages(sc, dtype, lists=False):
    return helpers.oracle_stages(sc.g, sc.cam, sc.T, sc.near, sc.far, sc.pad, dtype, mh=sc.mh if lists else None)


def oracle_vjp(sc, st, slab):
    return helpers.oracle_vjp(st, slab)


def random_slab(V, seed):
    """[V, 9] render gradients whose rows' magnitudes spread over 1e-6 .. 1"""
    gen = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (-6.0 * torch.rand(V, 1, generator=gen, dtype=torch.float64))
    return (torch.randn(V, SLAB_WIDTH, generator=gen, dtype=torch.float64) * mag).float()


# ---- the error measure of the tests ---------------------------------------------------------------------------------
def r_measure(got, ref, env):
    """per element |got - ref| / (env + 2^-22 |ref| + 1e-7 max|ref column|) with env = |oracle_fp32 - ref| (the error
    the reference's own fp32 arithmetic makes on that element); -> the max over all elements (0 for no elements)"""
    if ref.numel() == 0:
        return 0.0
    got, ref, env = (x.detach().double().cpu().reshape(x.shape[0], -1) for x in (got, ref, env))
    colmax = ref.abs().max(dim=0, keepdim=True).values
    den = env.abs() + 2.0 ** -22 * ref.abs() + 1e-7 * colmax
    num = (got - ref).abs()
    r = torch.where(num == 0, torch.zeros_like(num), num / den)
    return float(r.max())


# ---- scenes seen through general cameras ----------------------------------------------------------------------------
# name: (W, H).  A landscape and a portrait frame, a size that is no multiple of 16, a frame one tile high and one
# one tile wide.
KINDS = {"landscape": (640, 480), "portrait": (360, 640), "odd": (517, 301), "one_tile_high": (701, 13),
         "one_tile_wide": (11, 500)}
STRESS = ("quat_norm", "log_scale", "needle_disc", "near_plane", "far_plane", "uv_edge", "opacity", "optical_axis")


def look_at_pose(gen, target, dist):
    """a camera dist away from target, looking at it from a random direction with a random roll ->
    (A [3,3] rows = camera axes in world, centre C)"""
    fwd = torch.randn(3, generator=gen, dtype=torch.float64)
    fwd = fwd / fwd.norm()
    C = target - dist * fwd
    helper = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64) if abs(float(fwd[2])) < 0.9 else \
        torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
    right = torch.linalg.cross(fwd, helper)
    right = right / right.norm()
    down = torch.linalg.cross(fwd, right)
    roll = 2 * math.pi * float(torch.rand(1, generator=gen, dtype=torch.float64))
    r2 = math.cos(roll) * right + math.sin(roll) * down
    d2 = torch.linalg.cross(fwd, r2)
    return torch.stack([r2, d2, fwd]), C


def general_camera_scene(seed, N, W=None, H=None, deg=0, kind="landscape", stress=True, fy_over_fx=None,
                         near=0.3, far=500.0, pad=100, mh=3.0):
    """N Gaussians in a cluster around a world point ~20 from the origin, seen by a camera that looks at it from a
    random direction with a random roll: fx = W U(0.6, 1.3), fy = fx U(0.8, 1.25) (or fx * fy_over_fx), principal
    point off-centre by up to 15 % per axis.  stress=True gives each row of STRESS 3 % of the Gaussians.
    -> SimpleNamespace(g, cam, T, W, H, deg, near, far, pad, mh, rows={stress row: indices}) on the CPU, fp32."""
    if W is None:
        W, H = KINDS[kind]
    gen = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    n = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    fx = W * (0.6 + 0.7 * float(u(1)))
    fy = fx * (fy_over_fx if fy_over_fx is not None else 0.8 + 0.45 * float(u(1)))
    cx = W * (0.5 + 0.3 * (float(u(1)) - 0.5))
    cy = H * (0.5 + 0.3 * (float(u(1)) - 0.5))
    target = n(3)
    target = 20.0 * target / target.norm()
    dist = 6.0 + 4.0 * float(u(1))
    A, C = look_at_pose(gen, target, dist)
    t = -A @ C
    # camera-frame construction: pixel position, depth; 1/6 of the centres beyond the image's edges
    z = dist * (0.3 + 2.2 * u(N))
    px = -0.1 * W + 1.2 * W * u(N)
    py = -0.1 * H + 1.2 * H * u(N)
    wide = u(N) < 0.15
    px = torch.where(wide, -pad - 0.2 * W + (1.4 * W + 2 * pad) * u(N), px)
    py = torch.where(wide, -pad - 0.2 * H + (1.4 * H + 2 * pad) * u(N), py)
    q = n(N, 4)
    log_s = torch.log(z[:, None] * (0.5 + 5.5 * u(N, 3)) / fx)
    logit = 2.0 * n(N, 1)
    rgb = u(N, 3) / SH_0
    sh = 0.05 * n(N, 3, (deg + 1) ** 2 - 1) if deg > 0 else None
    rows = {}
    if stress:
        perm = torch.randperm(N, generator=gen)
        k = max(1, int(0.03 * N))
        for i, name in enumerate(STRESS):
            rows[name] = perm[i * k:(i + 1) * k].sort().values
        m = len(rows["quat_norm"])
        r = rows["quat_norm"]
        q[r] = q[r] / q[r].norm(dim=1, keepdim=True) * (10.0 ** (-3 + 6 * u(m, 1)))
        q[r, 0] = -q[r, 0].abs()
        log_s[rows["log_scale"]] = -12.0 + 16.0 * u(m, 3)
        r = rows["needle_disc"]
        base = torch.log(z[r] * (0.5 + 2.5 * u(m)) / fx)
        ratio = torch.log(10.0 ** (4 * u(m)))
        axis = torch.randint(0, 3, (m,), generator=gen)
        needle = u(m) < 0.5
        s = base[:, None].repeat(1, 3)
        s[torch.arange(m), axis] += torch.where(needle, ratio, -ratio)
        log_s[r] = s
        sign = lambda: torch.where(u(m) < 0.5, -1.0, 1.0)
        # 1e-4.5 .. 1e-3 off the plane, scaled with the point's lateral reach (the fp32 transform's rounding grows
        # with it): the fp32 and fp64 cull decisions agree
        for name, plane in (("near_plane", near), ("far_plane", far)):
            r = rows[name]
            lateral = (px[r] - cx).abs() / fx + (py[r] - cy).abs() / fy
            z[r] = plane + sign() * 10.0 ** (-4.5 + 1.5 * u(m)) * (1 + lateral * plane)
        r = rows["uv_edge"]
        edge_u = torch.where(u(m) < 0.5, torch.full((m,), -float(pad)), torch.full((m,), float(W + pad)))
        edge_v = torch.where(u(m) < 0.5, torch.full((m,), -float(pad)), torch.full((m,), float(H + pad)))
        on_u = u(m) < 0.5
        px[r] = torch.where(on_u, edge_u + sign() * 10.0 ** (-2 + 2 * u(m)), px[r])
        py[r] = torch.where(on_u, py[r], edge_v + sign() * 10.0 ** (-2 + 2 * u(m)))
        logit[rows["opacity"]] = sign()[:, None] * (25.0 + 5.0 * u(m, 1))
        r = rows["optical_axis"]
        px[r], py[r] = cx, cy
    cam_pts = torch.stack([(px - cx) * z / fx, (py - cy) * z / fy, z], dim=1)
    xyz = cam_pts @ A + C        # A^T c + C: the world point whose camera-frame coordinates are c
    if stress:
        xyz[rows["optical_axis"]] = C + z[rows["optical_axis"], None] * A[2]
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3], T[:3, 3] = A, t
    K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float64)
    f32 = lambda x: None if x is None else x.float().contiguous()
    g = Gaussians(f32(xyz), f32(rgb), f32(logit), f32(log_s), f32(q), f32(sh))
    return SimpleNamespace(g=g, cam=Camera(W, H, f32(K)), T=f32(T), W=W, H=H, deg=deg, near=near, far=far, pad=pad,
                           mh=mh, rows=rows, kind=kind, seed=seed)


# ---- a scene whose extreme needles have a degenerate fp32 record determinant, by construction -------------------------
DET_CLASSES = ("zero", "neg", "noisy")
N_NEEDLES, N_CONTROLS, N_ANGLES = 48, 8, 64


def rot_to_quat(R):
    """(w, x, y, z) of rotation matrices R [M, 3, 3] (quat_to_rot's convention), float64"""
    r = lambda i, j: R[:, i, j]
    # the four rows of 4 q q^T from the matrix' entries; the one with the largest diagonal element is well conditioned
    cands = torch.stack([
        torch.stack([1 + r(0, 0) + r(1, 1) + r(2, 2), r(2, 1) - r(1, 2), r(0, 2) - r(2, 0), r(1, 0) - r(0, 1)], dim=1),
        torch.stack([r(2, 1) - r(1, 2), 1 + r(0, 0) - r(1, 1) - r(2, 2), r(0, 1) + r(1, 0), r(0, 2) + r(2, 0)], dim=1),
        torch.stack([r(0, 2) - r(2, 0), r(0, 1) + r(1, 0), 1 - r(0, 0) + r(1, 1) - r(2, 2), r(1, 2) + r(2, 1)], dim=1),
        torch.stack([r(1, 0) - r(0, 1), r(0, 2) + r(2, 0), r(1, 2) + r(2, 1), 1 - r(0, 0) - r(1, 1) + r(2, 2)], dim=1)],
        dim=1)                                                        # [M, 4 candidates, 4]
    best = torch.diagonal(cands, dim1=1, dim2=2).argmax(dim=1)
    q = cands[torch.arange(R.shape[0]), best]
    q = q / q.norm(dim=1, keepdim=True)
    assert float((quat_to_rot(q) - R).abs().max()) < 1e-6   # (R comes from the fp32 pose: orthonormal to 1e-7)
    return q


def needle_rows(sc, angles_deg):
    """the constructed Gaussians for in-plane angles angles_deg [M] (row m is slot m % (N_NEEDLES + N_CONTROLS)) ->
    xyz, quaternion, log_scale, logit [M, ...] float64.  Slot i < N_NEEDLES: a needle (even i: scales long, short,
    short) or a disc seen edge-on (odd i: long, short, long along the view axis) with log10 of the ratio stepped from
    3.5 to 4 and the long axis 1e4 pixels wide (a, c >= 1e7 at 25 .. 65 degrees); the other slots: controls, ratio 1e2.
    Centres on a grid over the middle 80 % of the image at depths 6 .. 16: every cull plane is far away."""
    M = angles_deg.numel()
    slot = torch.arange(M) % (N_NEEDLES + N_CONTROLS)
    T, K = sc.T.double(), sc.cam.K.double()
    A, t = T[:3, :3], T[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    col, row = (slot % 8).double(), (slot // 8).double()
    px = sc.W * (0.1 + 0.8 * (col + 0.37) / 8)
    py = sc.H * (0.1 + 0.8 * (row + 0.61) / 7)
    z = 6.0 + 10.0 * ((slot * 37) % (N_NEEDLES + N_CONTROLS)).double() / (N_NEEDLES + N_CONTROLS)
    cam_pts = torch.stack([(px - cx) * z / fx, (py - cy) * z / fy, z], dim=1)
    xyz = (cam_pts - t) @ A            # A^T (c - t)
    phi = torch.deg2rad(angles_deg.double())
    zero, one = torch.zeros(M, dtype=torch.float64), torch.ones(M, dtype=torch.float64)
    Rz = torch.stack([torch.cos(phi), -torch.sin(phi), zero, torch.sin(phi), torch.cos(phi), zero, zero, zero, one],
                     dim=1).view(M, 3, 3)
    q = rot_to_quat(A.T @ Rz)          # columns: the Gaussian's axes in the world
    is_needle = slot < N_NEEDLES
    ratio = torch.where(is_needle, 10.0 ** (3.5 + 0.5 * slot.double() / (N_NEEDLES - 1)), torch.full_like(z, 1e2))
    s_long = 1e4 * z / fx
    s_short = s_long / ratio
    disc = is_needle & (slot % 2 == 1)
    log_s = torch.log(torch.stack([s_long, s_short, torch.where(disc, s_long, s_short)], dim=1))
    logit = torch.where(is_needle, zero, -3.0 * one)[:, None]
    return xyz, q, log_s, logit


def det_classes(conic):
    """class of the fp32 render record of conic [V, 3] (fp32): "zero" det == 0, "neg" det < 0, "noisy" det equal to one
    ulp of a c while the exact a c - b^2 of the same a, b, c is 0.3 .. 3 ulps (and not that ulp), else "plain"; the
    record's arithmetic: a = conic0 + 1/4, b = conic1 / 2, c = conic2 + 1/4, det = fl(fl(a c) - fl(b b))"""
    k = conic.detach().cpu().float().numpy()
    a, b, c = k[:, 0] + np.float32(0.25), k[:, 1] * np.float32(0.5), k[:, 2] + np.float32(0.25)
    ac = a * c
    det = ac - b * b
    exact = a.astype(np.float64) * c.astype(np.float64) - b.astype(np.float64) ** 2
    ulp = np.spacing(np.abs(ac)).astype(np.float64)
    out = np.full(len(det), "plain", dtype=object)
    out[(det == ulp) & (exact >= 0.3 * ulp) & (exact <= 3 * ulp) & (exact != ulp)] = "noisy"
    out[det < 0] = "neg"
    out[det == 0] = "zero"
    return out


def fp32_oracle_conic(sc):
    """-> (keep [N] bool, conic [V, 3]) of the fp32 oracle chain: the default of degenerate_needle_scene's search"""
    st = oracle_stages(sc, torch.float32)
    return st["keep"], st["conic"]


def _with_rows(base, rows):
    xyz, q, log_s, logit = (x.float() for x in rows)
    g = base.g
    M = xyz.shape[0]
    gen = torch.Generator().manual_seed(9)
    rgb = (torch.rand(M, 3, generator=gen, dtype=torch.float64) / SH_0).float()
    out = SimpleNamespace(**vars(base))
    out.g = Gaussians(torch.cat([g.xyz, xyz]).contiguous(), torch.cat([g.rgb, rgb]).contiguous(),
                      torch.cat([g.opacity, logit]).contiguous(), torch.cat([g.scale, log_s]).contiguous(),
                      torch.cat([g.quaternion, q]).contiguous(), None)
    return out


def degenerate_needle_scene(seed=171, N=2000, conic_of=fp32_oracle_conic):
    """general_camera_scene(seed, N, kind="odd", stress=False)'s camera and cluster, degree 0, plus N_NEEDLES extreme
    needles and discs and N_CONTROLS well-conditioned controls (needle_rows) as the last rows.  Each needle's in-plane
    angle is 25 + 40 i / 47 degrees plus j * 0.01, j < N_ANGLES, and j is chosen by a search: all candidates go through
    conic_of (scene -> keep, conic of the visible rows; the fp32 oracle chain, or a kernel's own stage), slot i takes
    the first j whose record has class DET_CLASSES[i % 3], or j = 0.  Nothing random decides class membership.
    -> the scene, with .rows = {class: Gaussian indices}, .controls, .needles"""
    base = general_camera_scene(seed, N, kind="odd", stress=False)
    S = N_NEEDLES + N_CONTROLS
    slot = torch.arange(S)
    base_angle = torch.where(slot < N_NEEDLES, 25.0 + 40.0 * slot.double() / (N_NEEDLES - 1), torch.full((S,), 45.0, dtype=torch.float64))
    cand_angles = (base_angle[None, :] + 0.01 * torch.arange(N_ANGLES, dtype=torch.float64)[:, None]).reshape(-1)
    cand = _with_rows(base, needle_rows(base, cand_angles))
    keep, conic = conic_of(cand)
    assert bool(keep[N:].all()), "a constructed row is culled"
    vis_rank = torch.cumsum(keep.long(), 0) - 1
    cls = det_classes(conic)[vis_rank[N:].numpy()].reshape(N_ANGLES, S)
    chosen = torch.zeros(S, dtype=torch.long)
    for i in range(N_NEEDLES):
        hits = np.nonzero(cls[:, i] == DET_CLASSES[i % 3])[0]
        chosen[i] = int(hits[0]) if len(hits) else 0
    sc = _with_rows(base, needle_rows(base, base_angle + 0.01 * chosen.double()))
    keep, conic = conic_of(sc)
    final = det_classes(conic)[(torch.cumsum(keep.long(), 0) - 1)[N:].numpy()]
    assert all(final[i] == cls[int(chosen[i]), i] for i in range(S)), "a row's class depends on the other rows"
    sc.rows = {c: N + torch.tensor([i for i in range(N_NEEDLES) if final[i] == c], dtype=torch.long) for c in DET_CLASSES}
    sc.needles = N + torch.arange(N_NEEDLES)
    sc.controls = N + N_NEEDLES + torch.arange(N_CONTROLS)
    sc.control_classes = list(final[N_NEEDLES:])
    sc.deg = 0
    return sc


def to_device(sc, device):
    """the scene's Gaussians, camera and pose on `device` (fresh tensors)"""
    d = lambda x: None if x is None else x.detach().to(device).contiguous().clone()
    g = sc.g
    return Gaussians(d(g.xyz), d(g.rgb), d(g.opacity), d(g.scale), d(g.quaternion), d(g.sh)), \
        Camera(sc.W, sc.H, d(sc.cam.K)), d(sc.T)
