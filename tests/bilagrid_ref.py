"""Test infrastructure: the definition of the bilateral-grid slice (include/gsplat_hip.h, ABI 23) restated in plain
torch in a chosen dtype -- value, both gradients by their closed forms, the per-node sum of contribution magnitudes
(abs_sum, the noise scale of grad_grid), the total variation and its gradient -- plus the PyTorch grid_sample
compositions the restatement is itself checked against, the cases of the GPU test and its left-out rule."""
import functools

import torch

LUM = (0.299, 0.587, 0.114)

# (W, H) and (L, Hg, Wg) of tests/test_gpu_bilagrid.py: every grid on the first frame, the first two on every frame
FRAMES = ((70, 45), (517, 301), (11, 500), (701, 13))
GRIDS = ((8, 16, 16), (4, 5, 3), (2, 2, 2), (1, 1, 1), (8, 2, 2), (1, 16, 16))
CASES = tuple((f, g) for g in GRIDS for f in FRAMES if f == FRAMES[0] or g in GRIDS[:2])
LEFT_OUT_CAP = 0.01   # at most this share of a case's pixels may be left out of the grad_image comparison


def _xy_axis(N, n, dtype):
    """cell, next node and fraction of the N pixel centres on an axis of n nodes; the cell in integers"""
    p = torch.arange(N, dtype=torch.int64)
    if n < 2:
        return torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=dtype)
    i0 = torch.clamp(((2 * p + 1) * (n - 1)) // (2 * N), max=n - 2)
    rem = (2 * p + 1) * (n - 1) - 2 * N * i0
    return i0, i0 + 1, rem.to(dtype) / torch.tensor(2 * N, dtype=dtype)


def luma(image):
    return (LUM[0] * image[..., 0] + LUM[1] * image[..., 1]) + LUM[2] * image[..., 2]


def _z_axis(image, L):
    lum = luma(image)
    gz = lum.clamp(0, 1) * (L - 1)
    z0 = torch.clamp(torch.floor(gz).to(torch.int64), max=max(L - 2, 0))
    z1 = torch.clamp(z0 + 1, max=L - 1)
    opened = (lum > 0) & (lum < 1) & (L > 1)
    return z0, z1, gz - z0.to(image.dtype), opened


def _sample(grid, image):
    """-> A, dA/dgz [H, W, 12], the corner indices and fractions"""
    _, L, Hg, Wg = grid.shape
    H, W, _ = image.shape
    G = grid.permute(1, 2, 3, 0)
    x0, x1, fx = _xy_axis(W, Wg, grid.dtype)
    y0, y1, fy = _xy_axis(H, Hg, grid.dtype)
    z0, z1, fz, opened = _z_axis(image, L)
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    FX, FY = fx[None, :, None], fy[:, None, None]

    def plane(z):
        a00, a01, a10, a11 = G[z, Y0, X0], G[z, Y0, X1], G[z, Y1, X0], G[z, Y1, X1]
        a0, a1 = a00 + FX * (a01 - a00), a10 + FX * (a11 - a10)
        return a0 + FY * (a1 - a0)

    lo, hi = plane(z0), plane(z1)
    d = hi - lo
    return lo + fz[..., None] * d, d, (x0, x1, fx, y0, y1, fy, z0, z1, fz, opened)


def slice_ref(grid, image):
    A, _, _ = _sample(grid, image)
    A = A.reshape(*image.shape[:2], 3, 4)
    return ((A[..., 0] * image[..., 0:1] + A[..., 1] * image[..., 1:2]) + A[..., 2] * image[..., 2:3]) + A[..., 3]


def backward_ref(grid, image, grad_out, closed=None):
    """-> grad_image, grad_grid, abs_sum.  closed: [H, W] bool, pixels whose guidance term is taken as absent"""
    _, L, Hg, Wg = grid.shape
    H, W, _ = image.shape
    A, dA, (x0, x1, fx, y0, y1, fy, z0, z1, fz, opened) = _sample(grid, image)
    A, dA = A.reshape(H, W, 3, 4), dA.reshape(H, W, 3, 4)
    if closed is not None:
        opened = opened & ~closed
    inner = ((dA[..., 0] * image[..., 0:1] + dA[..., 1] * image[..., 1:2]) + dA[..., 2] * image[..., 2:3]) + dA[..., 3]
    dz = (L - 1) * (grad_out * inner).sum(-1)
    dz = torch.where(opened, dz, torch.zeros_like(dz))
    lum = torch.tensor(LUM, dtype=grid.dtype)
    grad_image = (A[..., :3] * grad_out[..., :, None]).sum(-2) + lum * dz[..., None]

    rgb1 = torch.cat([image, torch.ones(H, W, 1, dtype=grid.dtype)], -1)
    contrib = (grad_out[..., :, None] * rgb1[..., None, :]).reshape(H * W, 12)
    gg = torch.zeros(L * Hg * Wg, 12, dtype=grid.dtype)
    ab = torch.zeros(L * Hg * Wg, 12, dtype=grid.dtype)
    for zi, wz in ((z0, 1 - fz), (z1, fz)):
        for yi, wy in ((y0, 1 - fy), (y1, fy)):
            for xi, wx in ((x0, 1 - fx), (x1, fx)):
                w = (wz * (wy[:, None] * wx[None, :])).reshape(H * W, 1)
                node = ((zi * Hg + yi[:, None]) * Wg + xi[None, :]).reshape(H * W)
                gg.index_add_(0, node, w * contrib)
                ab.index_add_(0, node, (w * contrib).abs())
    shape = lambda t: t.t().reshape(12, L, Hg, Wg).contiguous()
    return grad_image, shape(gg), shape(ab)


def left_out(image64, L):
    """the rule for the pixels left out of the grad_image comparison: only dz jumps there, and an fp32 luma may fall
    on the other side of the jump"""
    lum = luma(image64.double())
    near_edge = (lum.abs() < 2.0 ** -19) | ((lum - 1).abs() < 2.0 ** -19)
    if L < 2:
        return near_edge
    gz = lum.clamp(0, 1) * (L - 1)
    node = torch.round(gz)
    near_node = ((gz - node).abs() < 2.0 ** -16) & (node > 0) & (node < L - 1)
    return near_edge | near_node


def tv_ref(grids):
    """-> value (0-d), gradient, of grids [B, 12, L, Hg, Wg]"""
    val = torch.zeros((), dtype=grids.dtype)
    grad = torch.zeros_like(grids)
    for ax in (2, 3, 4):
        n = grids.shape[ax]
        if n < 2:
            continue
        d = grids.narrow(ax, 1, n - 1) - grids.narrow(ax, 0, n - 1)
        val = val + (d * d).sum() / d.numel()
        grad.narrow(ax, 1, n - 1).add_(d * (2.0 / d.numel()))
        grad.narrow(ax, 0, n - 1).sub_(d * (2.0 / d.numel()))
    return val, grad


# ---- the PyTorch compositions -----------------------------------------------------------------------------------------
def slice_torch(grid, image):
    """grid_sample(mode="bilinear", align_corners=True, padding_mode="border") over (gx, gy, gz), then the affine"""
    _, L, Hg, Wg = grid.shape
    H, W, _ = image.shape
    dt = grid.dtype
    gx = (torch.arange(W, dtype=dt) + 0.5) / W * 2 - 1
    gy = (torch.arange(H, dtype=dt) + 0.5) / H * 2 - 1
    gz = luma(image).clamp(0, 1) * 2 - 1
    coords = torch.stack([gx[None, :].expand(H, W), gy[:, None].expand(H, W), gz], -1)[None, None]
    A = torch.nn.functional.grid_sample(grid[None], coords, mode="bilinear", align_corners=True, padding_mode="border")
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (A[..., :3] * image[..., None, :]).sum(-1) + A[..., 3]


def tv_torch(grids):
    """the index-select composition"""
    val = 0
    for ax in (2, 3, 4):
        n = grids.shape[ax]
        if n >= 2:
            hi = grids.index_select(ax, torch.arange(1, n))
            lo = grids.index_select(ax, torch.arange(0, n - 1))
            val = val + ((hi - lo) ** 2).mean()
    return val if torch.is_tensor(val) else grids.sum() * 0


# ---- the inputs of the GPU cases ---------------------------------------------------------------------------------------
def identity_grid(L, Hg, Wg, dtype=torch.float32):
    return torch.eye(3, 4, dtype=dtype).reshape(12, 1, 1, 1).repeat(1, L, Hg, Wg)


def patches(W, H):
    """(y, x, h, w) of the patch of exact zeros and the patch of exact ones (8x8 where the frame has room)"""
    h, w = min(8, H), min(8, W)
    return (min(H // 5, H - h), min(W // 5, W - w), h, w), (max(H - H // 5 - h, 0), max(W - W // 5 - w, 0), h, w)


@functools.lru_cache(maxsize=None)
def case_inputs(frame, grid_shape):
    """fp32 inputs of one case, as float64 and float32 tensors: (grid, image, grad_out)"""
    (W, H), (L, Hg, Wg) = frame, grid_shape
    gen = torch.Generator().manual_seed(1000 * W + 10 * H + L + Hg + Wg)
    grid = (identity_grid(L, Hg, Wg) + 0.3 * torch.randn(12, L, Hg, Wg, generator=gen)).float()
    image = (torch.rand(H, W, 3, generator=gen) * 1.3 - 0.15).float()
    (ya, xa, h, w), (yb, xb, _, _) = patches(W, H)
    image[ya:ya + h, xa:xa + w] = 0.0
    image[yb:yb + h, xb:xb + w] = 1.0
    grad_out = torch.randn(H, W, 3, generator=gen).float()
    return grid, image, grad_out


def patch_mask(W, H):
    m = torch.zeros(H, W, dtype=torch.bool)
    for (y, x, h, w) in patches(W, H):
        m[y:y + h, x:x + w] = True
    return m


@functools.lru_cache(maxsize=None)
def case_reference(frame, grid_shape):
    """computed once per case and shared, never modified: the float64 and float32 restatements.  The guidance term
    is taken as absent on the two patches in both (on the ones patch the float64 luma rounds to just below 1)."""
    grid, image, grad_out = case_inputs(frame, grid_shape)
    closed = patch_mask(*frame)
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        g, i, go = grid.to(dt), image.to(dt), grad_out.to(dt)
        gi, gg, ab = backward_ref(g, i, go, closed)
        out[name] = dict(value=slice_ref(g, i), grad_image=gi, grad_grid=gg, abs_sum=ab)
    # the patches hold exact values, not near ones: they stay in, compared with the guidance term absent
    out["left_out"] = left_out(image.double(), grid_shape[0]) & ~closed
    return out
