"""The closed form of camera_T_world's gradient, per Gaussian (test code only), and the error measure of its tests.

A, t: the rotation block and translation of camera_T_world, twelve free numbers.  For a visible Gaussian with world
position p, c = A p + t = (x, y, z), slab row (g_rgb 3 | g_opa 1 | g_u, g_v | g_c0, g_c1, g_c2), Sigma and J as in
tests/ref64.py and G = [[g_c0, g_c1], [g_c1, g_c2]]:

  gM    = 2 G (J A) Sigma                 (the gradient of the product J A; conic_1 = S_01 + S_10 puts g_c1 on both)
  gJ    = gM A^T
  g_cam = (gJ_02 (-fx / z^2),
           gJ_12 (-fy / z^2),
           gJ_00 (-fx / z^2) + gJ_11 (-fy / z^2) + gJ_02 (2 fx x / z^3) + gJ_12 (2 fy y / z^3))
          + (z > 0) (g_u fx / z,  g_v fy / z,  -g_u fx x / z^2 - g_v fy y / z^2)
  dL/dA = J^T gM + g_cam p^T,   dL/dt = g_cam

The colour columns do not enter: the SH view direction carries no gradient (ref64.py)."""
import torch

from .ref64 import quat_to_rot


def pose_terms(xyz, q, log_scale, T, K, slab, dtype):
    """[V, 3, 4] terms (dL/dA | dL/dt) of the V Gaussians given (their parameter rows and slab rows), evaluated in
    `dtype` from the inputs converted to it"""
    xyz, q, log_scale, T, K, slab = (x.detach().cpu().to(dtype) for x in (xyz, q, log_scale, T, K, slab))
    A, t = T[:3, :3], T[:3, 3]
    fx, fy = K[0, 0], K[1, 1]
    c = xyz @ A.T + t
    x, y, z = c.unbind(1)
    R = quat_to_rot(q)
    M = R * torch.exp(log_scale)[:, None, :]
    sigma = M @ M.transpose(1, 2)
    zero = torch.zeros_like(z)
    J = torch.stack([fx / z, zero, -fx * x / (z * z), zero, fy / z, -fy * y / (z * z)], dim=1).view(-1, 2, 3)
    g_u, g_v, g0, g1, g2 = (slab[:, k] for k in (4, 5, 6, 7, 8))
    G = torch.stack([g0, g1, g1, g2], dim=1).view(-1, 2, 2)
    gM = 2 * G @ (J @ A) @ sigma
    gJ = gM @ A.T
    z2, z3 = z * z, z * z * z
    front = (z > 0).to(dtype)
    g_cam = torch.stack([
        gJ[:, 0, 2] * (-fx / z2) + front * g_u * fx / z,
        gJ[:, 1, 2] * (-fy / z2) + front * g_v * fy / z,
        gJ[:, 0, 0] * (-fx / z2) + gJ[:, 1, 1] * (-fy / z2) + gJ[:, 0, 2] * (2 * fx * x / z3)
        + gJ[:, 1, 2] * (2 * fy * y / z3) + front * (-g_u * fx * x / z2 - g_v * fy * y / z2)], dim=1)
    dA = J.transpose(1, 2) @ gM + g_cam[:, :, None] * xyz[:, None, :]
    return torch.cat([dA, g_cam[:, :, None]], dim=2)


def pose_reference(xyz, q, log_scale, T, K, slab):
    """-> (sum of the float64 terms [3, 4], B = sum |t64| [3, 4], E = sum |t32 - t64| [3, 4]); the inputs are the
    float32 rows of the visible Gaussians"""
    t64 = pose_terms(xyz, q, log_scale, T, K, slab, torch.float64)
    t32 = pose_terms(xyz, q, log_scale, T, K, slab, torch.float32).double()
    return t64.sum(0), t64.abs().sum(0), (t32 - t64).abs().sum(0)


def pose_r(got, ref, B, E):
    """max over the twelve elements of |got - ref| / (E + 2^-22 B): the measure of ref64.r_measure with the magnitude of
    the sum's terms in place of |ref| (cancellation takes |ref| / B down to 2e-3 on these scenes).  got: [4, 4] or
    [3, 4]"""
    got = got.detach().double().cpu()[:3]
    num = (got - ref).abs()
    den = E + 2.0 ** -22 * B
    r = torch.where(num == 0, torch.zeros_like(num), num / den)
    return float(r.max()) if r.numel() else 0.0
