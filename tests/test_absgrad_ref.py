"""tests/absgrad_ref.py, the references of the per-pixel absolute uv gradient, held to tests/render_ref64.py on the CPU:
on every scene of render_scenes() with one coefficient the signed sum of the per-(pixel, entry) terms IS the walk
gradient of the centres, the absolute sum lies between its magnitude and the sum of the leaf magnitudes (abs_walk, the
denominator of the GPU test's noise measure), and every Gaussian a live pixel uses has some.  One symmetric Gaussian
between four pixels under a constant grad_image shows what the quantity is for: its signed sum cancels to rounding,
its absolute sum does not.  The float32 restatement's measure (the environment of tests/test_gpu_absgrad.py) is
reported per scene.  Measured here: signed against grad_walk 1.3e-16 at most; absgrad / |signed| 5.0 to 11.6 in the
median; absgrad / abs_walk at least 1.2e-2 (long_1100); restatement 7e-9 to 1.0e-6 (long_1100), the fp32 oracle's signed
g_uv 8e-9 to 1.5e-6 by the same measure; 3.3e-4 both in opaque_stack, whose final weights of 1e-4 the fp32 forward forms
as 1 - A."""
from types import SimpleNamespace

import pytest
import torch

from . import render_ref64 as R
from .absgrad_ref import absgrad_fp64, scene_absgrad
from .helpers import report, scaled_err
from .test_render_ref64 import FP64_BOUND

SCENES = list(R.render_scenes())


@pytest.mark.parametrize("name", SCENES)
def test_absgrad_reference_on_the_scenes(name):
    e = scene_absgrad(name)
    ref, absgrad, signed = e["ref"], e["absgrad"], e["signed"]
    walk = ref.grad_walk["g_uv"]
    err = scaled_err(signed, walk)
    used = ref.used
    ratio = (absgrad[used] / walk[used].abs().clamp(min=1e-300)).median()
    share = (absgrad[used] / ref.abs_walk["g_uv"][used]).min()
    report(f"absgrad_ref[{name}]", signed_vs_walk=err, median_abs_over_signed=float(ratio),
           min_abs_over_abs_walk=float(share), restated=e["measure_restated"], oracle_signed=e["measure_oracle"])
    assert err < FP64_BOUND, err
    slack = 1e-12 * ref.abs_walk["g_uv"]   # (rounding of two float64 sums of the same terms)
    assert bool((absgrad + slack >= walk.abs()).all())
    assert bool((ref.abs_walk["g_uv"] + slack >= absgrad).all())
    assert bool((absgrad >= 0).all()) and bool((absgrad[used] > 0).all())
    assert not absgrad[~used].any()
    # far from the signed gradient: a kernel that returned |sum| would not pass for this
    assert float(ratio) > 2.0


def test_symmetric_gaussian_cancels_in_the_signed_sum_only():
    """one Gaussian at (15.5, 15.5) on 32 x 32 (the corner of four tiles), constant grad_image, black background"""
    W = H = 32
    sc = SimpleNamespace(W=W, H=H, V=1, uv=torch.tensor([[15.5, 15.5]]), conic=torch.tensor([[9.0, 0.0, 9.0]]),
                         opacity=torch.tensor([[0.6]]), coeff16=torch.tensor([[[1.0], [2.0], [0.5]]]),
                         rays=torch.zeros(H, W, 3), grad_image=torch.ones(H, W, 3), bg=torch.zeros(3),
                         sorted_g=torch.zeros(4, dtype=torch.int32), ranges=torch.arange(5, dtype=torch.int32))
    ref = R.render_fp64(sc.uv, sc.opacity, R.scene_coeff(sc, 1), sc.conic, sc.rays, sc.ranges, sc.sorted_g, sc.bg, W, H,
                        R.FP32, sc.grad_image)
    assert not ref.fragile.any()
    ref.grad_image = sc.grad_image.double()
    absgrad, signed = absgrad_fp64(sc, ref)
    assert scaled_err(signed, ref.grad_walk["g_uv"]) < FP64_BOUND or float(ref.grad_walk["g_uv"].abs().max()) < 1e-13
    assert float(absgrad.min()) > 0.1                       # sum of 3.5 * 0.6 * ... over some hundred pixels
    assert float(signed.abs().max()) < 1e-12 * float(absgrad.min())
