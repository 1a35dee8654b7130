"""Bilateral-grid colour correction between the rendered image and the loss, over the C ABI (csrc/bilagrid.hip).

Per-image appearance compensation ("Bilateral Guided Radiance Field Processing"): every training image owns a small
grid [12, L, Hg, Wg] of 3x4 affine colour transforms, sampled at the pixel's position and luma and applied to its
colour, so that auto-exposure and white-balance drift of a capture are absorbed by the grid instead of being baked
into the Gaussians.  A grid of one node per axis is one global 3x4 affine per image (exposure compensation).

    slice(grid, image)             [12, L, Hg, Wg], [H, W, 3] -> [H, W, 3], differentiable in both
    total_variation_loss(grids)    the smoothness regulariser of a stack of grids, differentiable
    BilateralGrid(num_images)      the grids of a capture as a Parameter, initialised to the identity (a no-op)

        bil = BilateralGrid(len(train_images), device="cuda")
        image, mask, uv = fused.rasterize(...)
        image = bil(image, i)
        loss = train_ops.ssim_l1_loss(image, target) + 10 * bil.tv_loss()

The definition is in include/gsplat_hip.h (ABI 23); it equals torch's grid_sample(mode="bilinear", align_corners=True,
padding_mode="border") composition.  grad_grid is reduced without atomics: the same inputs give the same bits.
"""
import torch

from . import _hip


def _check(grid, image):
    if not (torch.is_tensor(grid) and torch.is_tensor(image)):
        raise RuntimeError("bilagrid.slice takes tensors")
    if grid.dtype != torch.float32 or image.dtype != torch.float32:
        raise RuntimeError("bilagrid.slice takes float32 tensors")
    if grid.dim() != 4 or grid.shape[0] != 12 or min(grid.shape) < 1:
        raise RuntimeError(f"bilagrid.slice: grid must be [12, L, Hg, Wg], got {tuple(grid.shape)}")
    if image.dim() != 3 or image.shape[2] != 3 or min(image.shape) < 1:
        raise RuntimeError(f"bilagrid.slice: image must be [H, W, 3], got {tuple(image.shape)}")
    if not (grid.is_cuda and image.is_cuda and grid.device == image.device):
        raise RuntimeError("bilagrid.slice: grid and image must be on one GPU device")


def _dims(grid, image):
    return image.shape[0], image.shape[1], grid.shape[1], grid.shape[2], grid.shape[3]


def slice_forward(grid, image):
    """the raw forward call on checked, contiguous tensors -> out [H, W, 3]"""
    out = torch.empty_like(image)
    p = _hip.ptr
    _hip.call("gs_bilagrid_slice", p(grid), p(image), *_dims(grid, image), p(out), _hip.current_stream())
    return out


def slice_backward(grid, image, grad_out, want_image=True, want_grid=True, grad_grid=None):
    """the raw backward call -> (grad_image or None, grad_grid or None); grad_grid: a buffer to write into (every
    element is written)"""
    dims = _dims(grid, image)
    grad_image = torch.empty_like(image) if want_image else None
    ws = None
    if want_grid:
        if grad_grid is None:
            grad_grid = torch.empty_like(grid)
        ws = torch.empty(max(_hip.lib().gs_bilagrid_workspace_bytes(*dims) // 4, 1), dtype=torch.float32,
                         device=grid.device)
    else:
        grad_grid = None
    p = _hip.ptr
    _hip.call("gs_bilagrid_slice_backward", p(grid), p(image), p(grad_out), *dims, p(ws), p(grad_image), p(grad_grid),
              _hip.current_stream())
    return grad_image, grad_grid


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, image):
        ctx.save_for_backward(grid, image)
        return slice_forward(grid, image)

    @staticmethod
    def backward(ctx, grad_out):
        grid, image = ctx.saved_tensors
        want_grid, want_image = ctx.needs_input_grad
        if not (want_grid or want_image):
            return None, None
        grad_image, grad_grid = slice_backward(grid, image, grad_out.contiguous(), want_image, want_grid)
        return grad_grid, grad_image


def slice(grid, image):   # noqa: A001 -- the operation's name in the literature
    """image' = A(p) (R, G, B, 1) with A the grid sampled at the pixel's position and luma.

    grid [12, L, Hg, Wg] (a view grids[i] of a stack is contiguous and is taken as it is), image [H, W, 3]: float32
    tensors on one GPU device, else RuntimeError before any device call.  Differentiable in both; when neither
    requires a gradient only the forward kernel is launched."""
    _check(grid, image)
    grid, image = grid.contiguous(), image.contiguous()
    if not (torch.is_grad_enabled() and (grid.requires_grad or image.requires_grad)):
        return slice_forward(grid.detach(), image.detach())
    return _Slice.apply(grid, image)


def tv_raw(grids, want_grad=True):
    """the raw call on a checked, contiguous [B, 12, L, Hg, Wg] stack -> (tv [1], grad or None)"""
    B, _, L, Hg, Wg = grids.shape
    ws = torch.empty(max(_hip.lib().gs_bilagrid_tv_workspace_bytes(B, L, Hg, Wg) // 8, 1), dtype=torch.float64,
                     device=grids.device)
    out = torch.empty(1, dtype=torch.float32, device=grids.device)
    grad = torch.empty_like(grids) if want_grad else None
    p = _hip.ptr
    _hip.call("gs_bilagrid_tv", p(grids), B, L, Hg, Wg, p(ws), p(out), p(grad), _hip.current_stream())
    return out, grad


class _TotalVariation(torch.autograd.Function):
    """value and gradient from one call; backward scales the stored gradient"""

    @staticmethod
    def forward(ctx, grids):
        out, ctx.grad = tv_raw(grids, grids.requires_grad)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if ctx.grad is None or g is None:
            return None
        return ctx.grad * g


def total_variation_loss(grids):
    """sum over the three grid axes of two or more nodes of the mean squared difference of adjacent nodes, over all
    grids and channels of grids [B, 12, L, Hg, Wg] (or one grid [12, L, Hg, Wg]) -> 0-d tensor, differentiable"""
    if not (torch.is_tensor(grids) and grids.is_cuda and grids.dtype == torch.float32):
        raise RuntimeError("bilagrid.total_variation_loss takes a float32 device tensor")
    if grids.dim() == 4:
        grids = grids.unsqueeze(0)
    if grids.dim() != 5 or grids.shape[1] != 12 or min(grids.shape) < 1:
        raise RuntimeError(f"bilagrid.total_variation_loss: grids must be [B, 12, L, Hg, Wg], got {tuple(grids.shape)}")
    return _TotalVariation.apply(grids.contiguous())


class BilateralGrid(torch.nn.Module):
    """the grids of num_images training images: self.grids is a Parameter [num_images, 12, grid_l, grid_y, grid_x],
    every node the identity affine, so a fresh module returns the image's bits"""

    def __init__(self, num_images, grid_x=16, grid_y=16, grid_l=8, device=None):
        super().__init__()
        eye = torch.eye(3, 4, dtype=torch.float32, device=device).reshape(1, 12, 1, 1, 1)
        self.grids = torch.nn.Parameter(eye.repeat(num_images, 1, grid_l, grid_y, grid_x))

    def forward(self, image, index):
        return slice(self.grids[index], image)

    def tv_loss(self):
        return total_variation_loss(self.grids)
