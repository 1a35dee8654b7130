"""Shared test helpers: fixture loading and scene construction."""
import os

import numpy as np
import torch

from gaussian_splatting_amd.splat_py.structs import Camera, Gaussians

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SH_0 = 0.28209479177387814


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def t(a, device="cpu", dtype=None):
    x = torch.from_numpy(np.asarray(a))
    if dtype is not None:
        x = x.to(dtype)
    return x.to(device).contiguous()


def scene_from_fixture(fx, device="cpu", requires_grad=False, opacity_key="in_opacity"):
    def p(key):
        x = t(fx[key], device)
        return x.requires_grad_(True) if requires_grad else x

    sh = p("in_sh") if "in_sh" in fx.files else None
    g = Gaussians(p("in_xyz"), p("in_rgb"), p(opacity_key), p("in_scale"), p("in_quaternion"), sh)
    cam = Camera(int(fx["in_width"]), int(fx["in_height"]), t(fx["in_K"], device))
    return g, cam, t(fx["in_camera_T_world"], device)


def scene6(device="cpu"):
    """The reference's 6-Gaussian test scene (test/gaussian_test_data.py:6-86), from the fixture;
    opacity already passed through inverse_sigmoid as test_rasterize.py:18 does."""
    fx = load("ref_host_scene6.npz")
    return scene_from_fixture(fx, device, opacity_key="in_opacity_logit") + (fx,)


def rel_err(g, ref, floor_frac=1e-2):
    """Element-wise relative error max |g - ref| / max(|ref|, floor_frac * max|ref|).

    The floor is needed because per-Gaussian gradients are fp32 sums over pixels in an unspecified
    order (warp reduce + atomicAdd in the reference, wave reduce + atomics here): an element that
    is a near-cancelling sum carries the rounding noise of its largest terms (measured: 5e-7 of the
    tensor's max), so its relative error is unbounded as it approaches zero.  With the floor at 1 %
    of the tensor's max the measured error is 3e-5; at 1e-6 (the floor SURVEY.md 8(d) proposed) it
    is 1e-2 for the same data -- reorder noise, not a kernel difference."""
    g = g.detach().double().cpu()
    ref = ref.detach().double().cpu()
    if ref.numel() == 0:
        return 0.0
    floor = floor_frac * ref.abs().max().item()
    den = torch.clamp(ref.abs(), min=max(floor, 1e-300))
    return ((g - ref).abs() / den).max().item()


def scaled_err(g, ref):
    """max |g - ref| / max|ref| -- error relative to the tensor's scale"""
    g = g.detach().double().cpu()
    ref = ref.detach().double().cpu()
    if ref.numel() == 0:
        return 0.0
    return ((g - ref).abs().max() / ref.abs().max().clamp(min=1e-300)).item()


def noise_normalised_err(g, ref, abs_sum):
    """max over ALL elements (no floor) of |g - ref| / abs_sum.

    `abs_sum` is the oracle's sum, over the pixels that contribute to a gradient element, of the
    magnitudes of the LEAF terms of its formula -- every product that enters a sum or a difference
    (oracle.gs_oracle.render_tiles_backward_abs).  It is the scale of the unavoidable fp32 noise of that
    element: a different but equally valid fp32 evaluation (other factoring, reciprocal instead of
    division, another summation order -- the reference's own warp reduce + atomicAdd has that freedom)
    deviates from the oracle's value by a few 2^-24 of it, whatever cancels afterwards.  A correct kernel
    therefore stays within ~1e-5 of every element's own scale, including the small, cancelling elements
    that `rel_err`'s floor lets through."""
    g = g.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().cpu().reshape(-1)
    a = abs_sum.detach().double().cpu().reshape(-1)
    if ref.numel() == 0:
        return 0.0
    touched = a > 0
    assert not g[~touched].any(), "gradient on an element that no pixel contributes to"
    if not touched.any():
        return 0.0
    return ((g - ref).abs()[touched] / a[touched]).max().item()


# ---- parity report: numbers the GPU tests measured, printed at the end of the run and written to
# gpurun_out/parity_report.json (tests/conftest.py) -------------------------------------------------------
REPORT = []


def report(test, **values):
    REPORT.append(dict(test=test, **{k: (float(v) if isinstance(v, (int, float)) else v) for k, v in values.items()}))


def grad_errors(g, ref, abs_sum=None):
    """the three error measures of one gradient tensor: SURVEY.md 8(d)'s (floor 1e-6 of the max), the
    1 %-floor form the assertions use, the error relative to the tensor's scale, and -- when the oracle's
    abs-sums are given -- the floor-free noise-normalised error"""
    out = {"rel_floor_1e-6": rel_err(g, ref, 1e-6), "rel_floor_1e-2": rel_err(g, ref, 1e-2), "scaled": scaled_err(g, ref)}
    if abs_sum is not None:
        out["noise_normalised"] = noise_normalised_err(g, ref, abs_sum)
    return out


# ---- the oracle's per-stage kernels (oracle/gs_oracle.cpp) chained, in either precision ------------------------------
def _oracle():
    from oracle import gs_oracle
    gs_oracle.set_modes(0, 0)
    gs_oracle.set_sh_band1_mode(0)
    return gs_oracle


def oracle_stages(g, cam, T, near, far, pad, dtype=torch.float32, mh=None):
    """The per-Gaussian stage restated on the CPU with the oracle's kernels (CPU tensors g, cam.K, T).  The
    world->camera transform is the kernels' explicit expression ((m0 x + m1 y) + m2 z) + m3, the cull compares with
    the thresholds as `dtype` values, the SH colour is taken from the camera centre -A^-1 t formed in double.  fp32:
    the HIP stage's bits (the colour up to the centre's last ulp); fp64: an independent derivation next to
    tests/ref64.py.  mh given: also the oracle's sorted tile lists (fp32 only).  -> culled [N], keep, V and, per visible
    Gaussian, uv, xyz_c, conic, opacity [V,1], rgb, plus what oracle_vjp needs."""
    orc = _oracle()
    T, K = T.detach().to(dtype).contiguous(), cam.K.detach().to(dtype).contiguous()
    xyz = g.xyz.detach().to(dtype)
    x, y, z = xyz.unbind(1)
    xyz_c = torch.stack([T[i, 0] * x + T[i, 1] * y + T[i, 2] * z + T[i, 3] for i in range(3)], dim=1).contiguous()
    N = xyz.shape[0]
    uv = torch.zeros(N, 2, dtype=dtype)
    orc.camera_projection_cuda(xyz_c, K, uv)
    f = lambda v: torch.tensor(float(np.float32(v)), dtype=dtype)
    culled = ((xyz_c[:, 2] < f(near)) | (xyz_c[:, 2] > f(far)) | (uv[:, 0] < f(-1.0 * pad)) |
              (uv[:, 0] > f(cam.width + pad)) | (uv[:, 1] < f(-1.0 * pad)) | (uv[:, 1] > f(cam.height + pad)))
    keep = ~culled
    V = int(keep.sum())
    uv, xc = uv[keep].contiguous(), xyz_c[keep].contiguous()
    q, s = g.quaternion.detach()[keep].to(dtype).contiguous(), g.scale.detach()[keep].to(dtype).contiguous()
    sigma = torch.zeros(V, 3, 3, dtype=dtype)
    orc.compute_sigma_world_cuda(q, s, sigma)
    J = torch.zeros(V, 2, 3, dtype=dtype)
    orc.compute_projection_jacobian_cuda(xc, K, J)
    conic = torch.zeros(V, 3, dtype=dtype)
    orc.compute_conic_cuda(sigma, J, T, conic)
    logit = g.opacity.detach()[keep].to(dtype).contiguous()
    opacity = orc.sigmoid_det(logit) if dtype == torch.float32 else torch.sigmoid(logit)
    A = T[:3, :3].double().numpy()
    center = torch.from_numpy(-np.linalg.inv(A) @ T[:3, 3].double().numpy()).to(dtype)
    Minv = torch.eye(4, dtype=dtype)
    Minv[:3, 3] = center
    xyz_v = xyz[keep].contiguous()
    rgb = g.rgb.detach()[keep].to(dtype).contiguous()
    if g.sh is not None:
        coeffs = torch.cat((rgb.unsqueeze(2), g.sh.detach()[keep].to(dtype)), dim=2).contiguous()
        rgb = torch.zeros(V, 3, dtype=dtype)
        orc.precompute_rgb_from_sh_cuda(xyz_v, coeffs, Minv, rgb)
    out = dict(culled=culled, keep=keep, V=V, uv=uv, xyz_c=xc, conic=conic, opacity=opacity, rgb=rgb, sigma=sigma, J=J,
               q=q, s=s, Minv=Minv, T=T, K=K, xyz_v=xyz_v, N=N, n_coeff=1 if g.sh is None else g.sh.shape[2] + 1)
    if mh is not None:
        ntx, nty = (cam.width + 15) // 16, (cam.height + 15) // 16
        out["sorted"], out["ranges"] = orc.get_sorted_gaussian_list(1024, uv, xc, conic, ntx, nty, mh)
    return out


def oracle_vjp(st, slab):
    """dense parameter gradients (xyz, quaternion, scale, opacity, rgb[, sh]) from the render-gradient slab [V, 9]
    (rgb 3 | opacity 1 | uv 2 | conic 3) of the visible rows of oracle_stages' st: the oracle's per-stage backward
    kernels chained as the reference's autograd graph chains them (cuda_autograd_functions.py:19-219 + the glue of
    rasterize.py:29-99), in st's precision"""
    orc = _oracle()
    dtype, V, N, n_coeff = st["uv"].dtype, st["V"], st["N"], st["n_coeff"]
    slab = slab.to(dtype)
    g_rgb, g_opa = slab[:, 0:3].contiguous(), slab[:, 3:4].contiguous()
    g_uv, g_conic = slab[:, 4:6].contiguous(), slab[:, 6:9].contiguous()
    z = lambda *shape: torch.zeros(*shape, dtype=dtype)
    g_sigma, g_J = z(V, 3, 3), z(V, 2, 3)
    orc.compute_conic_backward_cuda(st["sigma"], st["J"], st["T"], g_conic, g_sigma, g_J)
    g_q, g_s = z(V, 4), z(V, 3)
    orc.compute_sigma_world_backward_cuda(st["q"], st["s"], g_sigma, g_q, g_s)
    gx1, gx2 = z(V, 3), z(V, 3)
    orc.compute_projection_jacobian_backward_cuda(st["xyz_c"], st["K"], g_J, gx1)
    orc.camera_projection_backward_cuda(st["xyz_c"], st["K"], g_uv, gx2)
    g_xyz = (gx1 + gx2) @ st["T"][:3, :3]   # rows: R^T g
    g_coeff = z(V, 3, n_coeff)
    if n_coeff > 1:
        orc.precompute_rgb_from_sh_backward_cuda(st["xyz_v"], st["Minv"], g_rgb, g_coeff)
    else:
        g_coeff[:, :, 0] = g_rgb   # degree 0: the colour is the rgb parameter itself
    y = st["opacity"].reshape(-1, 1)
    g_logit = g_opa * (1 - y) * y
    keep = st["keep"]

    def dense(v, shape):
        out = z(*shape)
        out[keep] = v
        return out

    out = dict(xyz=dense(g_xyz, (N, 3)), quaternion=dense(g_q, (N, 4)), scale=dense(g_s, (N, 3)),
               opacity=dense(g_logit, (N, 1)), rgb=dense(g_coeff[:, :, 0], (N, 3)))
    if n_coeff > 1:
        out["sh"] = dense(g_coeff[:, :, 1:], (N, 3, n_coeff - 1))
    return out
