"""The inputs of the depth / alpha tests (tests/depth_alpha_ref.py: render_ref64's scenes with a seeded z as the colour)
are fit for what tests/test_gpu_depth_alpha.py asks of them; CPU only.

  * few pixels are fragile, so the comparison covers the scenes;
  * on every scene that has scaled pixels the reference WALK's gradient (what the colour backward returns, SURVEY.md
    Q1 / Q4) lies far from the true derivative in the measure the GPU test uses -- a depth backward that walked like
    the colour backward could not pass it;
  * the fp32 oracle, which supplies the GPU test's envelope and baseline, takes the reference's decisions.

Measured here (noise_measure of grad_walk against grad, the minimum over the four tensors per scene):
  partial_48x40 7.2e-2, partial_33x17 2.3e-2, strip_70x13 4.3e-2, partial_48x40_black 8.1e-2, faint_300 3.3e-3,
  long_1100 2.7e-3, edge_cases_32x16 3.5e-3; opaque_stack has no scaled pixel.  Fragile pixels: none.
  fp32 oracle against the reference: depth within 7.5e-6 (long_1100), alpha within 4.4e-7; against the true
  derivative on the unscaled pixels 6.4e-6 (long_1100), 3.3e-4 in opaque_stack."""
import pytest
import torch

from . import depth_alpha_ref as D
from . import render_ref64 as R
from .test_render_ref64 import oracle_run

SCENES = list(R.render_scenes())
WALK_IS_NOT_THE_DERIVATIVE = 1e-3


@pytest.mark.parametrize("name", SCENES)
def test_fragile_pixels_are_few(name):
    ref = D.reference(name)
    assert float(ref.fragile.float().mean()) <= 0.02
    assert not ref.grad_image[ref.fragile].any() and not ref.grad_image[..., 2].any()
    assert float(ref.depth.max()) > 0 and float(ref.alpha.max()) > 0
    # z is 1 .. 10 and the weights sum to alpha: the depth map is a weighted mean of z times alpha
    assert bool((ref.depth >= ref.alpha * 1.0 - 1e-12).all()) and bool((ref.depth <= ref.alpha * 10.0 + 1e-12).all())


def test_some_scenes_have_scaled_pixels_and_one_has_none():
    share = {name: float((D.reference(name).scale != 1).float().mean()) for name in SCENES}
    assert share["opaque_stack"] == 0.0
    assert sum(v > 0.05 for v in share.values()) >= 6, share


@pytest.mark.parametrize("name", SCENES)
def test_walk_gradient_is_told_from_the_derivative(name):
    ref = D.reference(name)
    if not bool((ref.scale != 1).any()):
        for k in D.KEYS:
            assert D.noise_measure(ref.grad_walk[k], ref.grad[k], ref.abs[k]) < 1e-14, k
        return
    for k in D.KEYS:
        m = D.noise_measure(ref.grad_walk[k], ref.grad[k], ref.abs[k])
        assert m > WALK_IS_NOT_THE_DERIVATIVE, (name, k, m)


@pytest.mark.parametrize("name", SCENES)
def test_oracle_takes_the_reference_decisions(name):
    """the fp32 oracle on the depth scene: num_splats equal on the non-fragile pixels, and on the pixels with
    scale == 1 its (walk) gradient is the true derivative up to fp32 noise -- the baseline of the GPU test's rule (a)"""
    sc = D.depth_scene(name)
    ref, true = D.reference(name), D.reference(name, True)
    orc = oracle_run(sc, 1, torch.float32, true.grad_image, exact=True)
    ok = ~ref.fragile
    assert torch.equal(orc["nsp"][ok], ref.nsp[ok])
    got = D.fields(orc)
    for k in D.KEYS:
        assert D.noise_measure(got[k], true.grad[k], true.abs[k]) < WALK_IS_NOT_THE_DERIVATIVE, k
