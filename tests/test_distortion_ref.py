"""The reference of the depth-distortion tests (tests/distortion_ref.py) is fit for what tests/test_gpu_distortion.py
asks of it; CPU only.

  * its gradient is the derivative of its forward: central finite differences in float64, decisions held;
  * on a z-sorted list the list-order form IS the pairwise form sum_{i,j} w_i w_j |z_i - z_j| -- and on the scenes'
    own, unsorted z it is not, so a kernel that sorted or took |.| could not pass;
  * few pixels are fragile, and every scene has contributors on both sides of a chunk boundary where its list allows;
  * the fp32 restatement, the GPU test's yardstick, is an fp32 evaluation of the same thing: close to the reference in
    the GPU test's own measures.

Measured here: finite differences within 9.0e-10 of the sum of the directional derivative's term magnitudes (bound
1e-7: h = 1e-6, truncation h^2 and rounding 1e-16 / h); list order against pairwise on sorted z within 4.2e-15 of the
largest value (bound 1e-13), on the scenes' own z apart by 1.0 to 1.7 of it; fragile pixels: none on all eight
scenes; the restatement's noise_measure against the reference 1.5e-6 at most (long_1100, g_z; 2.7e-7 on the slab's
columns), its forward within 6.7e-7 of abs_p (edge_cases_32x16).  long_1100: 1100 walked entries, up to 546
contributors per pixel; faint_300: 300 walked, up to 196."""
import pytest
import torch

from . import depth_alpha_ref as D
from . import distortion_ref as X
from . import render_ref64 as R

SCENES = list(R.render_scenes())
ONE_TILE = [n for n in SCENES if R.render_scenes()[n].ranges.numel() == 2]
FRAGILE_SHARE = 0.01


@pytest.mark.parametrize("name", ["partial_33x17", "edge_cases_32x16"])
def test_reference_gradient_equals_finite_differences(name):
    sc, ref = D.depth_scene(name), X.reference(name)
    gi = ref.grad_image
    leaves = dict(g_z=sc.z.double(), g_opacity=sc.opacity.double(), g_uv=sc.uv.double(), g_conic=sc.conic.double())

    def loss(at):
        dist, depth, alpha, _ = X.composite(sc, at["g_uv"], at["g_opacity"], at["g_conic"], at["g_z"], ref.decisions)
        return float((dist * gi[..., 0] + depth * gi[..., 1] + alpha * gi[..., 2]).sum())

    gen = torch.Generator().manual_seed(77)
    h = 1e-6
    for k in X.KEYS:   # one leaf at a time, three random directions each
        assert float(ref.grad[k].abs().max()) > 0, k
        for _ in range(3):
            d = torch.randn(leaves[k].shape, generator=gen, dtype=torch.float64)
            fd = (loss(dict(leaves, **{k: leaves[k] + h * d})) - loss(dict(leaves, **{k: leaves[k] - h * d}))) / (2 * h)
            want = float((ref.grad[k] * d).sum())
            scale = float((ref.grad[k] * d).abs().sum())
            print(f"finite differences[{name}, {k}]: {abs(fd - want) / scale:.3g}")
            assert abs(fd - want) <= 1e-7 * scale, (k, fd, want, scale)


@pytest.mark.parametrize("name", ONE_TILE)
def test_list_order_form_is_the_pairwise_form_on_a_sorted_list(name):
    sc, ref = D.depth_scene(name), X.reference(name)
    z_sorted = torch.sort(sc.z.double()).values   # the one-tile lists hold the splats in index order
    assert torch.equal(sc.sorted_g.long(), torch.arange(sc.V))
    f = lambda x: x.double()
    dist = X.composite(sc, f(sc.uv), f(sc.opacity), f(sc.conic), z_sorted, ref.decisions)[0]
    pair = X.pairwise(sc, ref.decisions, z_sorted)
    top = float(pair.max())
    print(f"list order - pairwise[{name}]: {float((dist - pair).abs().max()) / top:.3g} of the largest value")
    assert top > 0 and float((dist - pair).abs().max()) <= 1e-13 * top, float((dist - pair).abs().max()) / top
    assert bool((dist >= 0).all())
    # the scenes' own z is not sorted: there the list-order form is another number
    own = X.pairwise(sc, ref.decisions)
    assert float((ref.distortion - own).abs().max()) > 1e-2 * float(own.max())


@pytest.mark.parametrize("name", SCENES)
def test_scenes_are_fit_for_the_comparison(name):
    sc, ref = D.depth_scene(name), X.reference(name)
    assert float(ref.fragile.float().mean()) <= FRAGILE_SHARE
    assert not ref.grad_image[ref.fragile].any()
    for ch in range(3):   # distortion, depth and alpha each have a gradient
        assert float(ref.grad_image[..., ch].abs().max()) > 0, ch
    assert float(ref.distortion.abs().max()) > 0 and float(ref.abs_p.max()) > 0
    assert bool((ref.abs_p >= ref.distortion.abs() * (1 - 1e-12)).all())
    assert bool(torch.allclose(ref.depth, D.reference(name).depth, rtol=1e-13, atol=1e-15))
    assert bool(torch.allclose(ref.alpha, D.reference(name).alpha, rtol=1e-13, atol=1e-15))
    # contributors on both sides of every chunk boundary the walked list crosses (64: the backward's, 256: the forward's)
    for tile, (contrib, n_walk) in ref.decisions.items():
        L = contrib.shape[1]
        any_c = contrib.any(dim=0)
        if name in ("long_1100", "faint_300"):
            assert int(n_walk.max()) == L == {"long_1100": 1100, "faint_300": 300}[name]
            for edge in range(64, L, 64):
                assert bool(any_c[edge - 64:edge].any()) and bool(any_c[edge:edge + 64].any()), (name, edge)
    if name == "long_1100":
        assert int(next(iter(ref.decisions.values()))[0].sum(dim=1).max()) == 546   # contributors of one pixel


@pytest.mark.parametrize("name", SCENES)
def test_restatement_is_an_fp32_evaluation_of_the_reference(name):
    ref = X.reference(name)
    ok = ~ref.fragile
    fwd = float(((ref.rest["distortion"].double() - ref.distortion).abs()[ok] / ref.abs_p[ok].clamp(min=1e-300)).max())
    assert fwd <= 1e-5, fwd
    for k, field in (("depth", ref.depth), ("alpha", ref.alpha), ("t_end", ref.t_end)):
        assert float((ref.rest[k].double() - field).abs().max()) <= 1e-4, k
    for k in X.KEYS:
        m = X.noise_measure(ref.rest[k], ref.grad[k], ref.abs[k])
        assert m <= 2e-5, (k, m)
        assert not ref.rest[k][~ref.used].any() and not ref.grad[k][~ref.used].any(), k
