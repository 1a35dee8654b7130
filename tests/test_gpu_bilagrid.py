"""The bilateral-grid kernels (csrc/bilagrid.hip, ABI 23) on the GPU against the float64 restatement of their definition
(tests/bilagrid_ref.py), with the project's standing measures:

  value, grad_image   ref64.r_measure with env = |restatement in fp32 - restatement in fp64|, bound R_MAX = 8
                      (tests/test_gpu_general_cameras.py); grad_image on the pixels the left-out rule keeps, the guidance
                      term taken as absent on the clamped pixels and on the patches of exact zeros and ones
  grad_grid           noise_measure (tests/test_gpu_render_ref64.py): the kernel may exceed the fp32 restatement's value of
                      the same measure by NOISE_MARGIN = 2e-5 and no more; nodes nobody contributes to are exact zeros
                      in a buffer that held NaN

plus the bit-level properties: two calls give the same bits, an identity grid returns the image, a NULL output leaves the
other one's bits alone, size-1 axes and constant grids have total variation exactly 0."""
import pytest
import torch

from gaussian_splatting_amd import bilagrid

from . import bilagrid_ref as B
from .helpers import report
from .ref64 import r_measure

pytestmark = pytest.mark.gpu

R_MAX = 8.0          # tests/test_gpu_general_cameras.py
NOISE_MARGIN = 2e-5  # tests/test_gpu_render_ref64.py
DEV = "cuda:0"


def noise_measure(got, ref, abs_sum):
    """max |got - ref| / abs_sum over the elements somebody contributes to (0 if none); tests/test_gpu_render_ref64.py"""
    a = abs_sum.double().reshape(-1)
    d = (got.double().reshape(-1) - ref.double().reshape(-1)).abs()
    return float((d[a > 0] / a[a > 0]).max()) if bool((a > 0).any()) else 0.0


@pytest.mark.parametrize("frame,grid_shape", B.CASES)
def test_slice_and_its_backward_against_the_reference(frame, grid_shape):
    ref = B.case_reference(frame, grid_shape)
    f64, f32 = ref["f64"], ref["f32"]
    grid, image, grad_out = (t.to(DEV) for t in B.case_inputs(frame, grid_shape))
    vals = {}

    out = bilagrid.slice_forward(grid, image).cpu()
    vals["r_value"] = r_measure(out, f64["value"], f32["value"].double() - f64["value"])

    buf = torch.full_like(grid, float("nan"))
    grad_image, grad_grid = bilagrid.slice_backward(grid, image, grad_out, grad_grid=buf)
    assert grad_grid is buf
    gi, gg = grad_image.cpu(), grad_grid.cpu()
    keep = ~ref["left_out"]
    vals["left_out"] = int(ref["left_out"].sum())
    vals["r_grad_image"] = r_measure(gi[keep], f64["grad_image"][keep],
                                     f32["grad_image"].double()[keep] - f64["grad_image"][keep])
    vals["noise_fp32_reference"] = noise_measure(f32["grad_grid"], f64["grad_grid"], f64["abs_sum"])
    vals["noise_kernel"] = noise_measure(gg, f64["grad_grid"], f64["abs_sum"])
    unreached = f64["abs_sum"] == 0
    vals["unreached_elements"] = int(unreached.sum())

    again_image, again_grid = bilagrid.slice_backward(grid, image, grad_out)
    only_image, none_grid = bilagrid.slice_backward(grid, image, grad_out, want_grid=False)
    none_image, only_grid = bilagrid.slice_backward(grid, image, grad_out, want_image=False)
    report(f"bilagrid_slice[{frame[0]}x{frame[1]}, grid {grid_shape}]", **vals)
    print(vals)

    assert vals["left_out"] <= B.LEFT_OUT_CAP * keep.numel()
    assert vals["r_value"] <= R_MAX, vals
    assert vals["r_grad_image"] <= R_MAX, vals
    assert not torch.isnan(gg).any(), "grad_grid has elements the backward did not write"
    assert vals["noise_kernel"] <= vals["noise_fp32_reference"] + NOISE_MARGIN, vals
    assert not gg[unreached].any(), "gradient on a node that no pixel reaches"
    assert gg[~unreached].abs().max() > 0
    # the same inputs give the same bits, whichever outputs are asked for
    assert torch.equal(again_image, grad_image) and torch.equal(again_grid, grad_grid)
    assert none_grid is None and none_image is None
    assert torch.equal(only_image, grad_image) and torch.equal(only_grid, grad_grid)


@pytest.mark.parametrize("frame", B.FRAMES)
def test_identity_grid_returns_the_image(frame):
    _, image, _ = B.case_inputs(frame, B.GRIDS[0])
    image = image.to(DEV)
    for shape in (B.GRIDS[0], B.GRIDS[1], (1, 1, 1)):
        out = bilagrid.slice(B.identity_grid(*shape).to(DEV), image)
        assert torch.equal(out, image), shape


@pytest.mark.parametrize("n_grids", (3, 1))
@pytest.mark.parametrize("grid_shape", B.GRIDS)
def test_total_variation_against_the_reference(grid_shape, n_grids):
    gen = torch.Generator().manual_seed(11 + n_grids)
    grids = (B.identity_grid(*grid_shape)[None] + 0.3 * torch.randn(n_grids, 12, *grid_shape, generator=gen)).float()
    want, want_grad = B.tv_ref(grids.double())
    g32 = grids.clone().requires_grad_(True)
    v32 = B.tv_torch(g32)    # the fp32 PyTorch composition: its error is the envelope
    v32.backward()
    tv, grad = bilagrid.tv_raw(grids.to(DEV))
    tv_only, no_grad = bilagrid.tv_raw(grids.to(DEV), want_grad=False)
    col = lambda t: t.detach().double().cpu().reshape(-1, 1)
    vals = dict(r_value=r_measure(col(tv), col(want), col(v32) - col(want)),
                r_grad=r_measure(col(grad), col(want_grad), col(g32.grad) - col(want_grad)))
    report(f"bilagrid_tv[{n_grids} grids {grid_shape}]", tv=float(tv), **vals)
    print(vals)
    assert no_grad is None and torch.equal(tv_only, tv)
    assert vals["r_value"] <= R_MAX and vals["r_grad"] <= R_MAX, vals
    if max(grid_shape) == 1:   # every axis has one node: exact zeros, whatever the values
        assert float(tv) == 0.0 and not grad.any()
    # a size-1 axis contributes exact zero: the value is that of the other axes alone, and a grid constant along them
    # has total variation 0 and gradient 0 exactly
    const = grids[:, :, :1, :1, :1].expand_as(grids).contiguous().to(DEV)
    tv0, grad0 = bilagrid.tv_raw(const)
    assert float(tv0) == 0.0 and not grad0.any()


def test_total_variation_loss_is_differentiable():
    gen = torch.Generator().manual_seed(5)
    grids = torch.randn(2, 12, 3, 4, 5, generator=gen).to(DEV).requires_grad_(True)
    loss = 10 * bilagrid.total_variation_loss(grids)
    loss.backward()
    tv, grad = bilagrid.tv_raw(grids.detach())
    assert loss.dim() == 0 and torch.equal(loss.detach(), 10 * tv[0])
    assert torch.equal(grids.grad, grad * 10)
    one = grids.detach()[0].clone().requires_grad_(True)   # [12, L, Hg, Wg] is a stack of one
    bilagrid.total_variation_loss(one).backward()
    assert torch.equal(one.grad, bilagrid.tv_raw(one.detach()[None])[1][0])


def test_autograd_through_the_module():
    frame, shape = B.FRAMES[0], B.GRIDS[0]
    grid, image, grad_out = (t.to(DEV) for t in B.case_inputs(frame, shape))
    bil = bilagrid.BilateralGrid(3, device=DEV)
    assert bil.grids.device.type == "cuda"
    with torch.no_grad():
        bil.grids[1] = grid
    img = image.clone().requires_grad_(True)
    out = bil(img, 1)
    out.backward(grad_out)
    want_image, want_grid = bilagrid.slice_backward(grid, image, grad_out)
    assert torch.equal(out.detach(), bilagrid.slice_forward(grid, image))
    assert not bil.grids.grad[0].any() and not bil.grids.grad[2].any()
    assert torch.equal(bil.grids.grad[1], want_grid)
    assert torch.equal(img.grad, want_image)
    # neither input requires a gradient: the forward alone, no graph
    assert not bilagrid.slice(grid, image).requires_grad


def test_a_short_fit_lowers_the_loss():
    """60 Adam steps on the grids alone, L1 to slice(grid_true, image) plus 10 tv: the loss must fall and stay finite.
    What the float64 CPU composition reaches from the same start is printed beside it; no ratio is fixed in advance."""
    (W, H), shape = B.FRAMES[0], (2, 4, 4)
    gen = torch.Generator().manual_seed(3)
    image = torch.rand(H, W, 3, generator=gen).float()
    grid_true = (B.identity_grid(*shape) + 0.3 * torch.randn(12, *shape, generator=gen)).float()
    target = B.slice_ref(grid_true.double(), image.double())

    def fit(params, loss_of):
        opt = torch.optim.Adam([params], lr=0.02)
        losses = []
        for _ in range(60):
            opt.zero_grad()
            loss = loss_of()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        return [float(x) for x in torch.stack(losses).cpu()]

    bil = bilagrid.BilateralGrid(1, grid_x=shape[2], grid_y=shape[1], grid_l=shape[0], device=DEV)
    img_d, tgt_d = image.to(DEV), target.float().to(DEV)
    got = fit(bil.grids, lambda: (bil(img_d, 0) - tgt_d).abs().mean() + 10 * bil.tv_loss())
    g64 = B.identity_grid(*shape, dtype=torch.float64)[None].clone().requires_grad_(True)
    img64 = image.double()
    cpu = fit(g64, lambda: (B.slice_torch(g64[0], img64) - target).abs().mean() + 10 * B.tv_torch(g64))
    report("bilagrid_fit[70x45, grid (2, 4, 4)]", first=got[0], last=got[-1], cpu64_first=cpu[0], cpu64_last=cpu[-1])
    print(f"loss {got[0]:.6g} -> {got[-1]:.6g}   float64 CPU composition {cpu[0]:.6g} -> {cpu[-1]:.6g}")
    assert all(x == x and abs(x) != float("inf") for x in got)
    assert bool(torch.isfinite(bil.grids).all())
    assert got[-1] < got[0]
