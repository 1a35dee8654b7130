"""The restatement of the bilateral-grid slice that the GPU test measures against (tests/bilagrid_ref.py), checked on
the CPU: against the float64 grid_sample composition with autograd, its total variation against the index-select
composition, the left-out share of every GPU case against its cap, and the GPU bounds against a correct but
differently ordered fp32 implementation (the fp32 grid_sample composition)."""
import pytest
import torch

from gaussian_splatting_amd import bilagrid  # noqa: F401 -- the feature under test; absent on the parent

from . import bilagrid_ref as B
from .ref64 import r_measure

R_MAX = 8.0   # tests/test_gpu_general_cameras.py
CHECK_GRIDS = ((8, 16, 16), (4, 5, 3), (1, 1, 1), (8, 2, 2))


def scaled(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


@pytest.mark.parametrize("grid_shape", CHECK_GRIDS)
def test_reference_equals_the_float64_grid_sample_composition(grid_shape):
    grid, image, grad_out = (t.double() for t in B.case_inputs(B.FRAMES[0], grid_shape))
    g, i = grid.clone().requires_grad_(True), image.clone().requires_grad_(True)
    want = B.slice_torch(g, i)
    want.backward(grad_out)
    grad_image, grad_grid, abs_sum = B.backward_ref(grid, image, grad_out)
    assert scaled(B.slice_ref(grid, image), want.detach()) < 1e-12
    assert scaled(grad_grid, g.grad) < 1e-12
    # dz jumps where the luma meets a node or the clamp; the composition's coordinate rounds differently there
    keep = ~B.left_out(image, grid_shape[0])
    assert float(keep.float().mean()) > 0.95
    assert scaled(grad_image[keep], i.grad[keep]) < 1e-12
    # the scale of a node's noise: no smaller than the node's sum, zero exactly where nothing contributes
    assert bool((abs_sum >= grad_grid.abs() * (1 - 1e-12)).all())


def test_clamped_pixels_carry_no_guidance_term():
    grid, image, grad_out = (t.double() for t in B.case_inputs(B.FRAMES[0], B.GRIDS[0]))
    lum = B.luma(image)
    clamped = (lum <= 0) | (lum >= 1)
    assert int((lum <= 0).sum()) >= 20 and int((lum >= 1).sum()) >= 20   # the inputs reach both sides of the clamp
    open_everywhere = B.backward_ref(grid, image, grad_out)[0]
    closed_there = B.backward_ref(grid, image, grad_out, closed=clamped)[0]
    assert torch.equal(open_everywhere, closed_there)


@pytest.mark.parametrize("n_grids", (3, 1))
@pytest.mark.parametrize("grid_shape", B.GRIDS)
def test_total_variation_equals_the_index_select_composition(grid_shape, n_grids):
    gen = torch.Generator().manual_seed(7)
    grids = torch.randn(n_grids, 12, *grid_shape, generator=gen, dtype=torch.float64)
    g = grids.clone().requires_grad_(True)
    want = B.tv_torch(g)
    want.backward()
    val, grad = B.tv_ref(grids)
    assert abs(float(val) - float(want.detach())) <= 1e-12 * max(abs(float(want.detach())), 1e-300)
    if max(grid_shape) > 1:
        assert scaled(grad, g.grad) < 1e-12
    else:
        assert float(val) == 0.0 and not grad.any()


@pytest.mark.parametrize("frame,grid_shape", B.CASES)
def test_left_out_share_stays_within_the_cap(frame, grid_shape):
    left = B.case_reference(frame, grid_shape)["left_out"]
    assert float(left.float().mean()) <= B.LEFT_OUT_CAP, int(left.sum())


@pytest.mark.parametrize("frame,grid_shape", [(B.FRAMES[0], g) for g in CHECK_GRIDS])
def test_a_differently_ordered_fp32_implementation_meets_the_gpu_bounds(frame, grid_shape):
    """the bound of tests/test_gpu_bilagrid.py must leave room for another correct fp32 evaluation: the fp32 grid_sample
    composition, which rounds its coordinates and its sums in another order, passes it on the 70x45 frame with the four
    grids the restatement itself is checked on (r <= 4.5 in value, <= 4.4 in grad_image).  It is not a tight
    implementation: it rounds the NORMALISED coordinate, which costs (n - 1) / 2 ulps of the cell fraction, and where
    the three colour terms cancel its worst element scores above the bound: 8.2 in value with grid (1, 16, 16) on this
    frame, 8.0 on 517x301 and 8.9 on 701x13 with (8, 16, 16), where the restatement in fp32, whose fractions are exact
    as the kernel's are, scores 0.9.  Those cases are therefore not asserted for the composition."""
    ref = B.case_reference(frame, grid_shape)
    grid, image, grad_out = B.case_inputs(frame, grid_shape)
    g, i = grid.clone().requires_grad_(True), image.clone().requires_grad_(True)
    got = B.slice_torch(g, i)
    got.backward(grad_out)
    f64, f32 = ref["f64"], ref["f32"]
    r_value = r_measure(got.detach(), f64["value"], f32["value"].double() - f64["value"])
    # the composition's own choice on the patches is not under test (it agrees on them: fp32 luma 0 and 1 exactly)
    keep = ~ref["left_out"]
    r_grad = r_measure(i.grad[keep], f64["grad_image"][keep], f32["grad_image"].double()[keep] - f64["grad_image"][keep])
    print(f"{frame} {grid_shape}: r_value {r_value:.3g}  r_grad_image {r_grad:.3g}")
    assert r_value <= R_MAX, r_value
    assert r_grad <= R_MAX, r_grad
