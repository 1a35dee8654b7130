"""tests/degenerate_det.py's scenes hold what they are aimed at, and the CPU oracle alone meets every criterion
tests/test_gpu_degenerate_det.py applies to the kernels: the classes are the ones asked for, every output is finite,
the det == 0 rows get exactly +0, nobody takes them (taking them out of the lists changes no bit), and the oracle's
gradients pass check_band_backward against themselves.  Also the scenes DESIGN.md 8 lists: the classes the oracle's
fp32 chain finds there, and that its render is finite with exact zeros on their det == 0 rows."""
import numpy as np
import pytest
import torch

from . import degenerate_det as D
from .helpers import grad_errors


def test_classes_are_exact_by_construction():
    for cls in D.CLASSES:
        for sign in (1.0, -1.0):
            conic = D.big_conic(cls, sign)
            assert D.classify([conic]) == [cls]
            a, b, c, det = D.record_abc([conic])
            assert a[0] >= 1e8 and c[0] >= 1e8 and np.sign(b[0]) == sign
    assert D.classify([D.SMALL["zero"], D.SMALL["neg"], (9.0, 2.0, 6.0)]) == ["zero", "neg", "plain"]
    for name, make in D.SCENES.items():
        sc = make()
        assert sc.got == sc.want, name
        assert all(len(sc.rows[cls]) >= 2 for cls in D.CLASSES) or name == "B"
    a = D.scene_a()
    assert a.ranges.numel() == 7 and a.V == 40 and sum(len(a.rows[c]) for c in D.CLASSES) == 12
    assert len(a.rows["zero"]) >= 4 and len(a.rows["neg"]) >= 4 and len(a.rows["noisy"]) >= 3


@pytest.mark.parametrize("name", list(D.SCENES))
@pytest.mark.parametrize("n_sh", [1, 4])
def test_oracle_meets_the_criteria(name, n_sh):
    sc = D.SCENES[name]()
    for exact in (True, False):
        ref = D.oracle_render(sc, n_sh, exact)
        assert bool(torch.isfinite(ref["image"]).all()) and bool(torch.isfinite(ref["fw"]).all())
        D.check_degenerate_gradients(sc, ref)
        for k in D.GRADS:   # nobody takes a det == 0 splat: not even a term magnitude
            assert not ref["a" + k[1:]].reshape(sc.V, -1)[sc.rows["zero"]].any(), k
            # the abs sums are sums of magnitudes on every row, the det < 0 rows (1 / det < 0) included, and no
            # gradient element is larger than its own sum of term magnitudes (up to the sum's rounding)
            a, g = ref["a" + k[1:]].double(), ref[k].double()
            assert bool((a >= 0).all()), k
            assert bool((g.abs() <= a * (1 + 1e-6)).all()), k
        # the small det < 0 records and the noisy ones on the screen ARE taken (the kernels' test would be empty
        # otherwise); a det < 0 record at needle magnitude is taken inside a wedge 1e-4 wide: by nobody
        big = sc.conic[:, 0] > 1e6
        for i in sc.rows["neg"][~big[sc.rows["neg"]]].tolist() + sc.rows["noisy"].tolist():
            if 0 <= float(sc.uv[i, 0]) < sc.W and 0 <= float(sc.uv[i, 1]) < sc.H:
                assert bool(ref["a_uv"][i].any()), i
        # without the det == 0 entries: the same bits (num_splats_per_pixel counts list entries: it changes)
        ref2 = D.oracle_render(D.without_rows(sc, sc.rows["zero"]), n_sh, exact)
        for k in ("image", "fw"):
            assert torch.equal(ref[k], ref2[k]), k
        if exact:
            for k in D.GRADS:
                assert torch.equal(ref[k], ref2[k]), k
        for k, a in zip(D.GRADS, ("a_rgb", "a_opa", "a_uv", "a_conic")):
            e = grad_errors(ref[k], ref[k], ref[a])
            assert e["noise_normalised"] == 0 and e["scaled"] == 0


def test_scene_b_walks_what_it_is_built_for():
    sc = D.scene_b()
    ref = D.oracle_render(sc)
    nsp = ref["nsp"]
    assert int(nsp.max()) == 150                                   # somebody walks the whole list: all chunks staged
    assert int(nsp.min()) <= max(D.B_STACK) + 1 < 40               # the corner stops at the opaque stack
    hit = ref["a_opa"].reshape(-1) > 0
    chunk = torch.arange(sc.V) // D.B_CHUNK
    assert not hit[chunk == 1].any()                               # a staged chunk nobody hits, with two det == 0 records
    assert set(sc.rows["zero"][chunk[sc.rows["zero"]] == 1].tolist()) == {100, 101}
    assert int(hit[chunk == 0].sum()) > 40 and int(hit[chunk == 2].sum()) > 10
    assert bool(hit[45]) and bool(hit[50])                         # the small det < 0 and the noisy record are taken


# ---- the scenes DESIGN.md 8 lists ------------------------------------------------------------------------------------
DESIGN8 = {162: dict(zero=[5445], neg=[1910]), 167: dict(zero=[217, 3253], neg=[])}


@pytest.mark.parametrize("seed", list(DESIGN8))
def test_design8_scenes_on_the_oracle(seed):
    from .ref64 import general_camera_scene, oracle_stages
    from .test_gpu_general_cameras import oracle_render
    sc = general_camera_scene(seed, 6000, kind="odd", stress=True)
    st = oracle_stages(sc, torch.float32, lists=True)
    _, _, _, det = D.record_abc(st["conic"].numpy())
    vis = torch.nonzero(st["keep"]).flatten()
    det = torch.from_numpy(det)
    assert vis[det == 0].tolist() == DESIGN8[seed]["zero"] and vis[det < 0].tolist() == DESIGN8[seed]["neg"]
    gen = torch.Generator().manual_seed(1)
    gi = (torch.randn(sc.H, sc.W, 3, generator=gen) / (sc.W * sc.H)).contiguous()
    ref = oracle_render(st, st["rgb"], torch.zeros(1, 1, 1), sc.W, sc.H, torch.full((3,), 0.5), gi)
    for k in ("image", "fw", "g_rgb", "g_opa", "g_uv", "g_conic"):
        assert bool(torch.isfinite(ref[k]).all()), k
    for k in ("g_rgb", "g_opa", "g_uv", "g_conic", "a_uv"):
        assert not ref[k][det == 0].any(), k


# ---- tests/ref64.py's constructed scene ------------------------------------------------------------------------------
def test_needle_scene_search_and_oracle_chain():
    """at least four rows of each class, none culled differently in fp64, controls well conditioned; the fp32 oracle
    chain alone is finite everywhere, leaves the det == 0 rows at exactly zero and meets r <= R_MAX"""
    from .ref64 import DET_CLASSES, degenerate_needle_scene, oracle_vjp
    from .test_gpu_general_cameras import R_MAX, Case, leaf_r, oracle_render
    sc = degenerate_needle_scene()
    assert all(len(sc.rows[c]) >= 4 for c in DET_CLASSES), {c: len(sc.rows[c]) for c in DET_CLASSES}
    assert all(c == "plain" for c in sc.control_classes)
    case = Case(sc, lists=True)
    assert bool(case.agree_v.all()) and bool(case.keep[sc.needles].all()) and bool(case.keep[sc.controls].all())
    st = case.st
    rank = torch.cumsum(case.keep.long(), 0) - 1
    c = st["conic"][rank[sc.needles]]
    assert float(c[:, 0].min()) >= 1e7 and float(c[:, 2].min()) >= 1e7
    gen = torch.Generator().manual_seed(2)
    gi = (torch.randn(sc.H, sc.W, 3, generator=gen) / (sc.W * sc.H)).contiguous()
    ref = oracle_render(st, st["rgb"], torch.zeros(1, 1, 1), sc.W, sc.H, torch.full((3,), 0.5), gi)
    for k, v in ref.items():
        assert not v.is_floating_point() or bool(torch.isfinite(v).all()), k
    zero_v = rank[sc.rows["zero"]]
    slab = torch.cat([ref["g_rgb"], ref["g_opa"], ref["g_uv"], ref["g_conic"]], dim=1)
    a_slab = torch.cat([ref["a_rgb"], ref["a_opa"], ref["a_uv"], ref["a_conic"]], dim=1)
    assert not slab[zero_v].any() and not a_slab[zero_v].any()
    for name in ("neg", "noisy"):   # these ARE taken
        assert bool((a_slab[rank[sc.rows[name]], 3] > 0).all()), name
    grads = oracle_vjp(sc, st, slab)
    for k, v in grads.items():
        assert bool(torch.isfinite(v).all()) and not v[sc.rows["zero"]].any(), k
    ok = torch.ones(sc.g.xyz.shape[0], dtype=torch.bool)
    rs = leaf_r(sc, case, lambda k: grads[k], slab, a_slab, ok)
    assert all(v <= R_MAX for v in rs.values()), rs
