"""The float64 reference of the per-Gaussian stage (tests/ref64.py) against two independent derivations: the oracle's
fp64 per-stage kernels, forward and chained backward, and finite differences (gradcheck).  Then the fp32 oracle
chain's per-element deviation from it -- the envelope the GPU tests measure the kernels against -- is finite and
bounded.  CPU only."""
import pytest
import torch

from .ref64 import (KINDS, LEAVES, STRESS, general_camera_scene, oracle_stages, oracle_vjp, per_gaussian_fp64,
                    random_slab, ref64_abs_vjp, ref64_stage)

FORWARD = (("uv", "uv"), ("xyz_cam", "xyz_c"), ("conic", "conic"), ("opacity_act", "opacity"), ("rgb_render", "rgb"))


def rel64(got, ref, floor=1e-9):
    """max per-element |got - ref| / (|ref| + floor * max|ref column|)"""
    got, ref = (x.double().reshape(x.shape[0], -1) for x in (got, ref))
    if ref.numel() == 0:
        return 0.0
    den = ref.abs() + floor * ref.abs().max(dim=0, keepdim=True).values
    num = (got - ref).abs()
    return float(torch.where(num == 0, torch.zeros_like(num), num / den).max())


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_ref64_equals_the_fp64_oracle_chain(kind, deg):
    sc = general_camera_scene(10 + deg, 3000, deg=deg, kind=kind)
    st = oracle_stages(sc, torch.float64)
    V = st["V"]
    assert 0 < V < 3000
    rows = torch.nonzero(st["keep"]).flatten()
    slab = random_slab(V, seed=deg)
    ref = ref64_stage(sc, slab, rows)
    assert torch.equal(ref["culled"], st["culled"])
    for k, ko in FORWARD:
        assert torch.isfinite(ref[k][rows]).all(), k
        assert rel64(st[ko], ref[k][rows]) < 1e-10, (k, rel64(st[ko], ref[k][rows]))
    orc = oracle_vjp(sc, st, slab)
    for k in orc:
        assert torch.isfinite(ref["grad"][k]).all(), k
        assert not ref["grad"][k][st["culled"]].any(), k
        assert rel64(orc[k], ref["grad"][k]) < 1e-10, (k, rel64(orc[k], ref["grad"][k]))


@pytest.mark.parametrize("row", STRESS)
def test_ref64_gradcheck_on_the_stress_rows(row):
    """autograd of ref64 against central differences on a handful of the visible Gaussians of each stress row"""
    sc = general_camera_scene(3, 2000, deg=3, kind="odd")
    ref = ref64_stage(sc)
    idx = sc.rows[row][~ref["culled"][sc.rows[row]]][:4]
    assert len(idx) > 0, row
    g = sc.g
    # each parameter row in units of its own magnitude, so that one finite-difference step suits quaternions of
    # norm 1e-3 and 1e3 alike
    x0 = [getattr(g, k).detach()[idx].double() for k in LEAVES]
    unit = [x.reshape(len(idx), -1).abs().amax(dim=1).clamp(min=1e-3).reshape((-1,) + (1,) * (x.dim() - 1)) for x in x0]
    params = [(x / m).clone().requires_grad_(True) for x, m in zip(x0, unit)]

    def y_of(*p):
        o = per_gaussian_fp64(*[x * m for x, m in zip(p, unit)], sc.T, sc.cam.K, sc.W, sc.H, sc.near, sc.far, sc.pad,
                              view_xyz=x0[0])   # (the view direction carries no gradient)
        return torch.cat([o["rgb_render"], o["opacity_act"], o["uv"], o["conic"]], dim=1)

    # outputs in units of each output column's magnitude at the point: one tolerance for every scale
    out_unit = y_of(*params).detach().abs().clamp(min=1e-30)
    assert torch.autograd.gradcheck(lambda *p: y_of(*p) / out_unit, params, eps=1e-7, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("kind", list(KINDS))
def test_fp32_oracle_envelope_is_finite_and_bounded(kind):
    """the fp32 oracle chain deviates from ref64 element by element by no more than its arithmetic explains: every
    element finite, within 10 % of its own magnitude plus 1e-5 of its column's largest (the bounds are loose; the GPU
    tests use the per-element envelope itself)"""
    sc = general_camera_scene(20, 4000, deg=3, kind=kind)
    st = oracle_stages(sc, torch.float32)
    rows = torch.nonzero(st["keep"]).flatten()
    slab = random_slab(st["V"], seed=1)
    ref = ref64_stage(sc, slab, rows)
    assert torch.equal(ref["culled"], st["culled"])
    for k, ko in FORWARD:
        assert torch.isfinite(st[ko]).all(), k
        assert rel64(st[ko], ref[k][rows], 1e-5) < 0.1, (k, rel64(st[ko], ref[k][rows], 1e-5))
    orc = oracle_vjp(sc, st, slab)
    for k in orc:
        assert torch.isfinite(orc[k]).all(), k
        assert rel64(orc[k], ref["grad"][k], 1e-5) < 0.1, (k, rel64(orc[k], ref["grad"][k], 1e-5))


def test_general_camera_scene_is_general():
    """the generator's cameras: fx != fy, principal point off-centre, a pose far from the identity, the cluster far
    from the origin; every stress row present and partly visible"""
    for kind, (W, H) in KINDS.items():
        sc = general_camera_scene(1, 2000, deg=2, kind=kind)
        K = sc.cam.K
        assert (sc.W, sc.H) == (W, H)
        assert abs(float(K[0, 0] / K[1, 1]) - 1) > 1e-3
        assert abs(float(K[0, 2]) - W / 2) > 1e-3 and abs(float(K[1, 2]) - H / 2) > 1e-3
        assert float((sc.T[:3, :3] - torch.eye(3)).abs().max()) > 0.1 and float(sc.T[:3, 3].norm()) > 5
        assert float(sc.g.xyz.mean(0).norm()) > 10
        culled = ref64_stage(sc)["culled"]
        for row in STRESS:
            assert len(sc.rows[row]) > 0 and not culled[sc.rows[row]].all(), (kind, row)
    K = general_camera_scene(1, 10, fy_over_fx=1.25).cam.K
    assert abs(float(K[1, 1] / K[0, 0]) - 1.25) < 1e-6


def test_abs_vjp_bounds_every_vjp_of_a_slab_within_the_term_magnitudes():
    """ref64_abs_vjp(a) bounds |VJP(slab)| element by element for any slab with |slab| <= a, and equals it for a slab
    with a single non-zero column"""
    sc = general_camera_scene(4, 1500, deg=3, kind="odd")
    rows = torch.nonzero(~ref64_stage(sc)["culled"]).flatten()
    slab = random_slab(len(rows), seed=2)
    bound = ref64_abs_vjp(sc, slab.abs(), rows)
    vjp = ref64_stage(sc, slab, rows)["grad"]
    for k in bound:
        assert bool((vjp[k].abs() <= bound[k] * (1 + 1e-12) + 1e-300).all()), k
    one = torch.zeros_like(slab)
    one[:, 7] = slab[:, 7]
    bound1, vjp1 = ref64_abs_vjp(sc, one.abs(), rows), ref64_stage(sc, one, rows)["grad"]
    for k in bound1:
        assert torch.allclose(bound1[k], vjp1[k].abs(), rtol=1e-12, atol=0), k
