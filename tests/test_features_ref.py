"""The inputs of the feature-map tests (tests/features_ref.py: render_ref64's scenes with seeded feature channels as
colours, three per reference call) are fit for what tests/test_gpu_features.py asks of them; CPU only.

  * few pixels are fragile, and the decisions (fragile, nsp, scale) are the same from channel group to channel group
    (tests/features_ref.reference_of asserts it while it combines them);
  * on every scene that has scaled pixels the reference WALK's gradient lies far from the true derivative in the measure
    the GPU test uses, in every tensor -- a feature backward that walked like the colour backward could not pass it;
  * the fp32 oracle, run group by group and combined the same way, takes the reference's decisions, and on the pixels
    with scale == 1 its gradient is the true derivative up to fp32 noise.

C = 5 (two groups, the second one holding two feature channels and alpha) on all eight scenes, C = 32 (eleven groups)
on partial_33x17.  (edge_cases_32x16 at C = 32 is not a case: with 33 channels of mixed sign summed into c_k its walk
gradient of g_opacity lies 9.1e-4 from the derivative, just under the constant; the GPU test does not rely on that
distance, its bounds are the oracle's noise + 2e-5.)
Measured here (noise_measure of grad_walk against grad, the minimum over the four tensors per scene, C = 5):
  partial_48x40 6.8e-2, partial_33x17 2.5e-2, strip_70x13 6.7e-2, partial_48x40_black 7.5e-2, faint_300 7.2e-3,
  long_1100 4.1e-3, edge_cases_32x16 5.0e-3; partial_33x17 at C = 32 8.8e-3; opaque_stack has no scaled pixel.
  Fragile pixels: none.
  fp32 oracle against the true derivative on the unscaled pixels: 6.5e-6 (long_1100, g_features), 7.0e-7 at most on
  the other scenes but opaque_stack, where it is 3.3e-4."""
import pytest
import torch

from . import features_ref as F
from . import render_ref64 as R
from .test_depth_alpha_ref import WALK_IS_NOT_THE_DERIVATIVE
from .test_render_ref64 import oracle_run

SCENES = list(R.render_scenes())
CASES = [(name, 5) for name in SCENES] + [("partial_33x17", 32)]


@pytest.mark.parametrize("name,C", CASES)
def test_fragile_pixels_are_few(name, C):
    ref = F.reference(name, C)
    assert float(ref.fragile.float().mean()) <= 0.02
    assert not ref.grad_image[ref.fragile].any()
    assert tuple(ref.feature_map.shape) == (ref.nsp.shape[0], ref.nsp.shape[1], C)
    assert float(ref.alpha.max()) > 0 and float(ref.feature_map.abs().max()) > 0
    for k, w in (("g_features", C), ("g_opacity", 1), ("g_uv", 2), ("g_conic", 3)):
        assert tuple(ref.grad[k].shape) == (R.render_scenes()[name].V, w), k


def test_some_scenes_have_scaled_pixels_and_one_has_none():
    share = {name: float((F.reference(name, 5).scale != 1).float().mean()) for name in SCENES}
    assert share["opaque_stack"] == 0.0
    assert sum(v > 0.05 for v in share.values()) >= 6, share


@pytest.mark.parametrize("name,C", CASES)
def test_walk_gradient_is_told_from_the_derivative(name, C):
    ref = F.reference(name, C)
    vals = {k: F.noise_measure(ref.grad_walk[k], ref.grad[k], ref.abs[k]) for k in F.KEYS}
    print(name, C, vals)
    if not bool((ref.scale != 1).any()):
        for k in F.KEYS:
            assert vals[k] < 1e-14, k
        return
    for k in F.KEYS:
        assert vals[k] > WALK_IS_NOT_THE_DERIVATIVE, (name, k, vals[k])


@pytest.mark.parametrize("name,C", CASES)
def test_oracle_takes_the_reference_decisions(name, C):
    """the fp32 oracle on the features scene: num_splats equal on the non-fragile pixels, and on the pixels with
    scale == 1 its combined (walk) gradient is the true derivative up to fp32 noise -- the baseline of the GPU test's
    rule (a)"""
    sc = F.features_scene(name, C)
    ref, true = F.reference(name, C), F.reference(name, C, True)
    orc = F.oracle_of(sc, true.grad_image, oracle_run)
    ok = ~ref.fragile
    assert torch.equal(orc["nsp"][ok], ref.nsp[ok])
    vals = {k: F.noise_measure(orc[k], true.grad[k], true.abs[k]) for k in F.KEYS}
    print(name, C, vals)
    for k in F.KEYS:
        assert vals[k] < WALK_IS_NOT_THE_DERIVATIVE, (k, vals[k])
