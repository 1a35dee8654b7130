"""tests/median_ref.py is fit to judge the median-depth kernels (no GPU needed): its depth / alpha are
depth_alpha_ref's, its float32 restatement takes the reference's median decision wherever the reference does not call
the pixel median-fragile, MEDIAN_MARGIN is eight times what that restatement's T_k needs, the median-fragile pixels
are few, and grad_z is what autograd makes of a gather.

The cap on the median-fragile share is a CONDITION on the scenes, not a tolerance of a kernel: a scene on which more
than 1 % of the pixels sit within 2^-17 of T_k = 0.5 would leave too little checked.  Measured: 0.39 % at most (one
pixel of 256 on long_1100), 0.05 % on partial_48x40_black (one of 1920), none elsewhere or on the constructed scenes."""
import pytest
import torch

from . import depth_alpha_ref as D
from . import median_ref as M
from . import render_ref64 as R

SCENES = list(R.render_scenes())
MAX_FRAGILE_SHARE = 0.01


def _restatement_agrees(sc, ref):
    ok = ~ref.median_fragile
    assert torch.equal(ref.rest.index[ok], ref.median_index[ok])
    assert ref.rest.t_deviation <= M.MEDIAN_MARGIN / 8, ref.rest.t_deviation
    share = float(ref.median_fragile.float().mean())
    assert share <= MAX_FRAGILE_SHARE, share
    return share


@pytest.mark.parametrize("name", SCENES)
def test_reference_on_the_scenes(name):
    sc, ref, base = D.depth_scene(name), M.reference(name), D.reference(name)
    # the same walk as depth_alpha_ref's: the same maps (another order of the float64 sums)
    assert float((ref.depth - base.depth).abs().max()) <= 1e-12 * max(1.0, float(base.depth.abs().max()))
    assert float((ref.alpha - base.alpha).abs().max()) <= 1e-12
    share = _restatement_agrees(sc, ref)
    print(f"median_ref[{name}]: T_k deviation {ref.rest.t_deviation:.3g}, median-fragile {100 * share:.2f} %")
    # the definition, restated per pixel on a few pixels by a plain loop
    z = sc.z.double()
    has = ref.median_index >= 0
    assert torch.equal(ref.median_depth[has], z[ref.median_index[has]]) and not ref.median_depth[~has].any()
    assert torch.equal(has, ref.alpha > 0)
    for tile, w in ref.walk.items():
        for p in range(0, w.px.numel(), 37):
            T, chosen, last = 1.0, -1, -1
            for k in range(w.idx.numel()):
                if bool(w.contrib[p, k]):
                    if T > 0.5:
                        chosen = k
                    last = k
                    T = T * (1 - float(w.alpha[p, k]))
            if chosen >= 0:
                # (the loop's product rounds in another order: its choice may differ only on a median-fragile pixel)
                if not bool(ref.median_fragile[w.py[p], w.px[p]]):
                    assert int(ref.median_index[w.py[p], w.px[p]]) == int(w.idx[chosen])
                if float(w.T_behind[p, chosen]) > 0.5 * (1 + M.MEDIAN_MARGIN):
                    assert chosen == last     # T never fell that far: the last contributor
            else:
                assert int(ref.median_index[w.py[p], w.px[p]]) == -1


@pytest.mark.parametrize("name", list(M.constructed()))
def test_reference_on_the_constructed_scenes(name):
    case, ref = M.constructed()[name], M.constructed_reference(name)
    _restatement_agrees(case.sc, ref)
    first = ref.median_index[:, :16]
    if case.expect is not None:
        assert bool((first == int(case.order[case.expect])).all()), name
    if name == "never_crosses":
        assert float(ref.alpha.max()) < 0.5
    if name == "nobody_reaches":
        assert bool((first == -1).any()) and bool((first >= 0).any()) and bool((ref.median_index[:, 16:] == -1).all())
        assert not ref.median_depth[ref.median_index < 0].any()
    if name == "saturates_early":
        assert int(ref.nsp.max()) < case.sc.V
    if name.startswith("crossing_at_"):
        assert int(ref.nsp.min()) == 300     # nobody stops: the crossing entry is reached across the chunk boundary


@pytest.mark.parametrize("name", ["partial_48x40", "opaque_stack", "edge_cases_32x16"])
def test_grad_z_is_the_gradient_of_a_gather(name):
    sc, ref = D.depth_scene(name), M.reference(name)
    z = sc.z.double().clone().requires_grad_(True)
    has = ref.median_index >= 0
    median_depth = torch.where(has, z[ref.median_index.clamp(min=0)], torch.zeros_like(ref.median_depth))
    (median_depth * ref.grad_median).sum().backward()
    assert float((z.grad - ref.grad_z).abs().max()) <= 1e-13 * max(1.0, float(ref.abs_z.max()))
    assert not z.grad[~ref.used].any() and bool(ref.used.any())
    assert not ref.grad_median[ref.fragile | ref.median_fragile].any()
