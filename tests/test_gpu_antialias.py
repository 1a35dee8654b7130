"""fused.rasterize(antialiased=True) / GS_RASTER_ANTIALIASED (ABI 14): the per-Gaussian kernels' antialiased
instantiations at the stage level, the frame through both orchestrations, what the factor is for (minification), a
short training run and the refusals.

Stage measures: ref64.r_measure with env = |the fp32 evaluation of the header's expressions on the fp32 oracle's conic and
opacity - the float64 reference| (tests/antialias_ref.py), bound R_MAX = 8 (tests/test_gpu_general_cameras.py).  Rows
whose `det_0 > 0` decision differs between fp32 and float64 (needles whose det_0 cancels: fp32 comp is off by orders of
magnitude there) are left out and must be fewer than 0.5 % of the visible rows.  Pose: the measure and bound of
tests/test_gpu_pose_grad.py.  Frame: tests/test_gpu_render_ref64.py's image measure, and for the parameter gradients
its noise rule one stage further down -- |got - ref| / (abs sums carried through the stage) may exceed the fp32 oracle
chain's value of the same measure by NOISE_MARGIN = 2e-5 and no more.

Measured on an MI355X (every case prints its figures and leaves them in the parity report):
  forward   r 1.0000 on all three scenes, cut and non-cut (the worst element IS the fp32 evaluation's own error);
            13 / 11 / 17 rows of 5 428 / 5 386 / 5 532 left out (the eight appended tiny rows among them)
  backward  whole set 0.19 .. 1.00, owner slice 0.18 .. 1.25
  pose      random slab 0.26 / 0.63 / 1.17; opacity column alone 0.58 / 0.19 / 0.36, the classic kernel 3e4 .. 1e5
  frame     r_image 1.20; parameter gradients: kernel 4.4e-6 .. 2.6e-5 against oracle 4.2e-6 .. 2.6e-5 (at most
            1.2e-7 above it), native and Python alike; alpha map r 2.06
  minification  R = 0.982 antialiased, 3.10 classic;  training: L1 0.0260 -> 0.0029 in 40 steps"""
import functools
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.splat_py.structs import Camera, Gaussians
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

from . import render_ref64 as R
from .antialias_ref import aa_terms, fold_slab, opacity_eff, opacity_eff_fp64
from .helpers import report
from .pose_terms import pose_r, pose_terms
from .ref64 import (LEAVES, SH_0, general_camera_scene, leaves64, oracle_stages, oracle_vjp, per_gaussian_fp64, r_measure,
                    random_slab, to_device)
from .test_gpu_render_ref64 import FRAME, NOISE_MARGIN, noise_measure
from .test_render_ref64 import oracle_run

pytestmark = pytest.mark.gpu
DEV = "cuda"
R_MAX = 8.0
N_STAGE = 6000
NAMES = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
AA, CLASSIC = 1, 0   # GS_RASTER_ANTIALIASED, GS_RASTER_CLASSIC (asserted against the header in test_forward)
LEFT_OUT_MAX = 0.005


def p(t):
    return None if t is None else t.data_ptr()


# ---- stage scenes ---------------------------------------------------------------------------------------------------
def with_tiny_rows(sc):
    """sc plus eight copies of Gaussians near the image centre, four with log-scale -20 and four with -50 (Sigma2D's
    determinant underflows in fp32: det_0 == 0)"""
    g = sc.g
    st = oracle_stages(sc, torch.float32)
    vis = torch.nonzero(st["keep"]).flatten()
    d = (st["uv"] - torch.tensor([sc.W / 2.0, sc.H / 2.0])).norm(dim=1)
    src = vis[d.argsort()[:8]]
    cat = lambda x: None if x is None else torch.cat([x, x[src].clone()], dim=0).contiguous()
    scale = cat(g.scale)
    scale[-8:-4] = -20.0
    scale[-4:] = -50.0
    sc.g = Gaussians(cat(g.xyz), cat(g.rgb), cat(g.opacity), scale, cat(g.quaternion), cat(g.sh))
    sc.tiny = torch.arange(g.xyz.shape[0], g.xyz.shape[0] + 8)
    return sc


@functools.lru_cache(maxsize=None)
def stage_case(kind, deg, seed):
    """scene, fp32 oracle stages, float64 stage and the rows both precisions decide alike on (cull and det_0 > 0)"""
    sc = with_tiny_rows(general_camera_scene(seed, N_STAGE, deg=deg, kind=kind))
    st = oracle_stages(sc, torch.float32, lists=True)
    keep, V = st["keep"], st["V"]
    vis_g = torch.nonzero(keep).flatten()
    L = leaves64(sc.g, requires_grad=False)
    ref = per_gaussian_fp64(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], sc.T, sc.cam.K, sc.W,
                            sc.H, sc.near, sc.far, sc.pad)
    cull_differs = (ref["culled"] != st["culled"])[vis_g]
    t32 = aa_terms(st["conic"], torch.float32)
    t64 = aa_terms(ref["conic"][vis_g], torch.float64)
    det_differs = (t32["det_0"] > 0) != (t64["det_0"] > 0)
    ok_v = ~(cull_differs | det_differs)
    n_out = int(det_differs.sum())
    assert n_out < LEFT_OUT_MAX * V, (n_out, V)
    return SimpleNamespace(sc=sc, st=st, V=V, vis_g=vis_g, ref=ref, ok_v=ok_v, t32=t32, n_det_differs=n_out,
                           opa32=opacity_eff(st["conic"], st["opacity"], torch.float32),
                           opa64=opacity_eff_fp64(ref["conic"][vis_g], ref["opacity_act"][vis_g]))


def stage_forward(sc, antialiased, cut):
    g, cam, T = to_device(sc, DEV)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, sc.near,
                                 sc.far, sc.pad, sc.mh, None, 0 if not cut else _hip.GS_SORT_PREFIX, depth_cut=cut,
                                 antialiased=antialiased)
    torch.cuda.synchronize()
    V = f.V
    c = lambda x: x[:V].detach().cpu()
    got = dict(uv=c(f.uv), xyz_cam=c(f.xyz_cam), conic=c(f.conic), opacity_act=c(f.opacity_act), rgb_render=c(f.rgb_render),
               packed=c(f.packed), vis_idx=c(f.vis_idx), culling_mask=f.culling_mask.cpu(), rank=f.rank.cpu(),
               ranges=f.ranges.cpu(), sorted_g=f.sorted_g.cpu())
    if cut:
        got["bin_rec"] = f.cut.bin_rec.view(-1, 8)[:V].cpu()
    return f, got, (g, cam, T)


def raw_forward(sc, g, cam, T, mode, cut=False):
    """gs_preprocess_forward_mode (mode None: gs_preprocess_forward_cut) through the typed loader on buffers of its
    own, the per-Gaussian entry point alone; cut: with bin_records, cut_workspace and depth_hist.
    -> (status, outputs by visible index as stage_forward names them, on the CPU; the raw buffers)"""
    lib = _hip.lib()
    N = g.xyz.shape[0]
    n_sh = 1 if g.sh is None else g.sh.shape[2] + 1
    T_ = ((sc.W + 15) // 16) * ((sc.H + 15) // 16)
    i32 = lambda n: torch.full((n,), -3, dtype=torch.int32, device=DEV)
    f32 = lambda *s: torch.full(s, 7.0, device=DEV)
    o = SimpleNamespace(ws=i32(lib.gs_preprocess_workspace_ints(N)), count=i32(1), rank=i32(N), vis=i32(N),
                        mask=torch.zeros(N, dtype=torch.uint8, device=DEV), center=f32(3), uv=f32(N, 2), xc=f32(N, 3),
                        conic=f32(N, 3), opa=f32(N, 1), rgb=f32(N, 3), packed=f32(N, 12),
                        bin_rec=f32(N, 8) if cut else None, cut_ws=i32(lib.gs_cut_workspace_ints(N, T_)) if cut else None,
                        hist=torch.zeros(_hip.GS_CUT_HIST_BINS, dtype=torch.int32, device=DEV) if cut else None)
    args = [p(g.xyz), p(g.quaternion), p(g.scale), p(g.opacity), p(g.rgb), p(g.sh), n_sh, p(T), p(cam.K), N, sc.W, sc.H,
            sc.near, sc.far, float(sc.pad), sc.mh, 0, (sc.H + 15) // 16, p(o.ws), p(o.center), p(o.count), p(o.mask),
            p(o.rank), p(o.vis), p(o.uv), p(o.xc), p(o.conic), p(o.opa), p(o.rgb), p(o.packed), p(o.bin_rec), p(o.cut_ws),
            p(o.hist), lib.gs_cut_sample_stride(N) if cut else 0]
    if mode is None:
        status = lib.gs_preprocess_forward_cut(*args, _hip.current_stream())
    else:
        status = lib.gs_preprocess_forward_mode(*args, mode, _hip.current_stream())
    torch.cuda.synchronize()
    if status != 0:
        return status, None, o
    V = int(o.count)
    c = lambda x: x[:V].cpu()
    got = dict(uv=c(o.uv), xyz_cam=c(o.xc), conic=c(o.conic), opacity_act=c(o.opa), rgb_render=c(o.rgb), packed=c(o.packed),
               vis_idx=c(o.vis), culling_mask=o.mask.cpu().bool(), rank=o.rank.cpu())
    if cut:
        got["bin_rec"] = c(o.bin_rec)
        assert not o.hist.any()   # returned to zero
    return status, got, o


@pytest.mark.parametrize("kind,deg", [("landscape", 3), ("odd", 0), ("one_tile_wide", 2)])
def test_forward(kind, deg):
    assert (_hip.GS_RASTER_ANTIALIASED, _hip.GS_RASTER_CLASSIC) == (AA, CLASSIC)
    case = stage_case(kind, deg, 130 + deg)
    sc, V = case.sc, case.V
    ntx, nty = (sc.W + 15) // 16, (sc.H + 15) // 16
    # the depth cut's binning serves the LDS-histogram regime (of these frames the one-tile-wide one): there the cut
    # form runs with its lists, elsewhere the per-Gaussian entry point's cut form alone
    cut_ok = bool(_hip.lib().gs_cut_supported(ntx, 0, nty, sc.g.xyz.shape[0]))
    assert cut_ok == (kind == "one_tile_wide")
    comp0 = case.t32["comp"] == 0
    assert int(comp0.sum()) >= 4 and bool(comp0[case.st["keep"].cumsum(0)[case.sc.tiny[-4:]] - 1].all())
    for cut in (False, True):
        if cut and not cut_ok:
            dev = to_device(sc, DEV)
            s0, classic, _ = raw_forward(sc, *dev, None, cut=True)
            s1, got, _ = raw_forward(sc, *dev, AA, cut=True)
            assert s0 == 0 and s1 == 0
        else:
            _, classic, _ = stage_forward(sc, False, cut)
            _, got, _ = stage_forward(sc, True, cut)
        assert got["packed"].shape[0] == V and set(got) == set(classic)
        assert torch.equal(got["conic"], case.st["conic"])   # the bits the fp32 evaluation below starts from
        for k in classic:
            if k != "packed":
                assert torch.equal(got[k], classic[k]), (cut, k)
        keep_cols = [0, 1] + list(range(4, 12))
        assert torch.equal(got["packed"][:, keep_cols], classic["packed"][:, keep_cols]), cut
        assert torch.equal(got["packed"][:, 7], case.t32["det_d"])
        opa = got["packed"][:, 3:4]
        ok = case.ok_v
        r = r_measure(opa[ok], case.opa64[ok], case.opa32[ok].double() - case.opa64[ok])
        same_bits = float((opa == case.opa32).float().mean())
        report(f"antialias_forward[{kind} deg {deg} cut {cut}]", r=r, left_out=case.n_det_differs, V=V,
               equal_to_fp32_evaluation=same_bits)
        print(f"antialias_forward[{kind} deg {deg} cut {cut}]: r = {r:.3g}, left out {case.n_det_differs} of {V}, "
              f"bits equal to the fp32 evaluation on {same_bits:.4f} of the rows")
        assert r <= R_MAX, r
        assert not got["packed"][comp0, 3].any() and bool((got["packed"][comp0, 2] == -1).all())
        # a smaller opacity never widens the cutoff radius
        assert bool((got["packed"][:, 2] <= classic["packed"][:, 2]).all())
        assert bool((got["packed"][:, 3] <= classic["packed"][:, 3]).all())


# ---- backward -------------------------------------------------------------------------------------------------------
def ref_backward(case, slab):
    """float64 autograd of (rgb | opa_eff | uv | conic) of the visible rows against slab, dense, keyed like LEAVES"""
    sc = case.sc
    L = leaves64(sc.g)
    out = per_gaussian_fp64(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], sc.T, sc.cam.K, sc.W,
                            sc.H, sc.near, sc.far, sc.pad)
    rows = case.vis_g
    y = torch.cat([out["rgb_render"][rows], opacity_eff_fp64(out["conic"][rows], out["opacity_act"][rows]),
                   out["uv"][rows], out["conic"][rows]], dim=1)
    keys = [k for k in LEAVES if L[k] is not None]
    grads = torch.autograd.grad(y, [L[k] for k in keys], grad_outputs=slab.double(), allow_unused=True)
    return {k: (torch.zeros_like(L[k]) if g is None else g) for k, g in zip(keys, grads)}


def backward_r(case, got, ref_g, env_g, i0=0, i1=None):
    N = case.sc.g.xyz.shape[0]
    i1 = N if i1 is None else i1
    ok = torch.ones(N, dtype=torch.bool)
    ok[case.vis_g[~case.ok_v]] = False
    ok = ok[i0:i1]
    culled = case.st["culled"][i0:i1]
    out = {}
    for k in got:
        if got[k] is None:
            continue
        assert not got[k][culled].any(), k
        r, e = ref_g[k][i0:i1], env_g[k][i0:i1].double()
        out[k] = r_measure(got[k][ok], r[ok], e[ok] - r[ok])
    return out


def check(tag, rs):
    report(tag, **rs)
    print(tag, {k: round(v, 3) for k, v in rs.items()})
    for k, v in rs.items():
        assert v <= R_MAX, (tag, k, v)


def raw_backward(entry, g, cam, T, f, slab, n_sh, extra):
    """one of the two backward entry points through the typed loader, status returned instead of raised"""
    N = g.xyz.shape[0]
    outs = [torch.full((N, w), 7.0, device=DEV) for w in (3, 4, 3, 1, 3)] + \
           [torch.full((N, 3, n_sh - 1), 7.0, device=DEV) if n_sh > 1 else None]
    args = [p(g.xyz), p(g.quaternion), p(g.scale), n_sh, p(T), p(cam.K), p(f.center), p(f.rank), p(f.opacity_act), p(slab),
            0, N] + [p(x) for x in outs] + list(extra) + [_hip.current_stream()]
    status = getattr(_hip.lib(), entry)(*args)
    torch.cuda.synchronize()
    return status, outs


@pytest.mark.parametrize("kind,deg", [("landscape", 3), ("odd", 0), ("one_tile_wide", 2)])
def test_backward(kind, deg):
    case = stage_case(kind, deg, 130 + deg)
    sc, V = case.sc, case.V
    N = sc.g.xyz.shape[0]
    tag = f"antialias_backward[{kind} deg {deg}]"
    slab = random_slab(V, 5)
    ref_g = ref_backward(case, slab)
    env_g = oracle_vjp(sc, case.st, fold_slab(case.st["conic"], case.st["opacity"], slab, torch.float32))
    f, _, (g, cam, T) = stage_forward(sc, True, False)
    slab_d = slab.to(DEV).contiguous()
    cpu = lambda out: {k: (None if x is None else x.cpu()) for k, x in zip(NAMES, out)}
    whole = cpu(fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab_d, antialiased=True))
    check(tag + " whole set", backward_r(case, whole, ref_g, env_g))
    comp0_g = case.vis_g[case.t32["comp"] == 0]
    assert comp0_g.numel() >= 4 and not whole["opacity"][comp0_g].any()
    # an owner slice: Gaussians [256, 1792), slab rows from v_base
    i0, i1 = 256, 1792
    v_base = int(case.st["keep"][:i0].sum())
    part = cpu(fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab_d[v_base:].contiguous(),
                                         v_base=v_base, i0=i0, i1=i1, antialiased=True))
    check(tag + " owner slice", backward_r(case, part, ref_g, env_g, i0, i1))
    for k in part:
        if part[k] is not None:
            assert torch.equal(part[k], whole[k][i0:i1]), k
    # the opacity column all zero: nothing to fold, the classic backward's bits
    zero3 = slab_d.clone()
    zero3[:, 3] = 0
    a = fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, zero3, antialiased=True)
    b = fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, zero3)
    for k, x, y in zip(NAMES, a, b):
        assert (x is None and y is None) or torch.equal(x, y), k
    # the factor is in it: with the opacity column alone the conic's parameters get a gradient
    only3 = torch.zeros_like(slab_d)
    only3[:, 3] = slab_d[:, 3]
    c = fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, only3, antialiased=True)
    d = fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, only3)
    assert bool(c[2].any()) and not bool(d[2].any())
    # GS_RASTER_CLASSIC through the new entry = the old entry; an unknown mode is refused
    n_sh = f.n_sh
    s_old, old = raw_backward("gs_preprocess_backward", g, cam, T, f, slab_d, n_sh, [])
    s_new, new = raw_backward("gs_preprocess_backward_mode", g, cam, T, f, slab_d, n_sh, [CLASSIC])
    assert s_old == 0 and s_new == 0
    for k, x, y in zip(NAMES, old, new):
        assert (x is None and y is None) or torch.equal(x, y), k
    s_bad, untouched = raw_backward("gs_preprocess_backward_mode", g, cam, T, f, slab_d, n_sh, [7])
    assert s_bad == _hip.GS_EINVAL and b"raster_mode" in _hip.lib().gs_last_error()
    assert all(x is None or bool((x == 7.0).all()) for x in untouched)


def test_forward_and_pose_modes_through_the_new_entries():
    """GS_RASTER_CLASSIC through gs_preprocess_forward_mode / gs_pose_backward_mode launches the old entries' kernels:
    equal bits; raster_mode 7 returns GS_EINVAL and writes nothing"""
    case = stage_case("odd", 0, 130)
    sc = case.sc
    f, classic, (g, cam, T) = stage_forward(sc, False, False)
    N = sc.g.xyz.shape[0]
    lib = _hip.lib()

    status, got, o = raw_forward(sc, g, cam, T, CLASSIC)
    assert status == 0 and int(o.count) == f.V
    V = f.V
    for k in got:
        assert torch.equal(got[k], classic[k]), k
    status, got, o = raw_forward(sc, g, cam, T, 7)
    assert status == _hip.GS_EINVAL and got is None and b"raster_mode" in lib.gs_last_error()
    assert bool((o.packed == 7.0).all()) and bool((o.rank == -3).all())
    # pose
    slab = random_slab(V, 6).to(DEV).contiguous()
    want = fused.pose_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab)

    def pose(mode, opacity_act):
        grad = torch.full((4, 4), 7.0, device=DEV)
        ws = torch.empty(lib.gs_pose_workspace_floats(N), device=DEV)
        args = [p(g.xyz), p(g.quaternion), p(g.scale), p(T), p(cam.K), p(f.rank), p(opacity_act), p(slab), 0, N, p(ws),
                p(grad), mode, _hip.current_stream()]
        status = lib.gs_pose_backward_mode(*args)
        torch.cuda.synchronize()
        return status, grad

    status, grad = pose(CLASSIC, None)
    assert status == 0 and torch.equal(grad, want)
    status, grad = pose(7, f.opacity_act)
    assert status == _hip.GS_EINVAL and bool((grad == 7.0).all())
    status, grad = pose(AA, None)
    assert status == _hip.GS_EINVAL and bool((grad == 7.0).all())


def pose_reference_aa(case, slab):
    """(autograd's dL/dT in float64 through the factor, and sum t64, B, E of the closed form of tests/pose_terms.py on
    the folded slab: folded in float64 from the float64 conic, in fp32 from the kernels' conic)"""
    sc, vis, g = case.sc, case.vis_g, case.sc.g
    L = leaves64(g, requires_grad=False)
    T64 = sc.T.double().clone().requires_grad_(True)
    out = per_gaussian_fp64(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], T64, sc.cam.K, sc.W,
                            sc.H, sc.near, sc.far, sc.pad)
    y = torch.cat([opacity_eff_fp64(out["conic"][vis], out["opacity_act"][vis]), out["uv"][vis], out["conic"][vis]], dim=1)
    (auto,) = torch.autograd.grad(y, T64, grad_outputs=slab[:, 3:].double())
    f64 = fold_slab(case.ref["conic"][vis], case.ref["opacity_act"][vis], slab, torch.float64)
    f32 = fold_slab(case.st["conic"], case.st["opacity"], slab, torch.float32)
    rows = (g.xyz[vis], g.quaternion[vis], g.scale[vis], sc.T, sc.cam.K)
    t64 = pose_terms(*rows, f64, torch.float64)
    t32 = pose_terms(*rows, f32, torch.float32).double()
    return auto, t64.sum(0), t64.abs().sum(0), (t32 - t64).abs().sum(0)


@pytest.mark.parametrize("kind,deg", [("landscape", 3), ("odd", 0), ("one_tile_wide", 2)])
def test_pose(kind, deg):
    """gs_pose_backward_mode against float64 autograd through the factor, by the measure of tests/test_gpu_pose_grad.py:
    r = |got - sum t64| / (E + 2^-22 B) over the per-Gaussian terms.  The terms are the closed form of
    tests/pose_terms.py on the folded slab; their float64 sum is first held to autograd of the whole stage.
    Two slabs.  The random one of the other stage tests: the factor's share of its sum is 1e-8 of B and less (measured on
    the CPU; the stress rows' conic terms set B), so it shows that nothing else moved.  Then the opacity column alone
    on the rows outside the log_scale / needle_disc stress rows (E / B 4e-6 to 1e-4 there; with those rows the fp32
    evaluation's own error on their cancelling det_0 takes E / B to 0.05 .. 0.2): the classic kernel, which never reads
    that column, returns exact zeros, which is r > 3e4 on the CPU."""
    case = stage_case(kind, deg, 130 + deg)
    sc, V, vis = case.sc, case.V, case.vis_g
    fwd, _, (gd, cam, T) = stage_forward(sc, True, False)
    run = lambda s, aa: fused.pose_backward(gd.xyz, gd.quaternion, gd.scale, T, cam.K, fwd, s.to(DEV).contiguous(),
                                            antialiased=aa)
    slab = random_slab(V, 17)
    slab[~case.ok_v] = 0   # rows the two precisions decide differently on carry nothing
    only3 = torch.zeros_like(slab)
    only3[:, 3] = slab[:, 3]
    stress = torch.zeros(sc.g.xyz.shape[0], dtype=torch.bool)
    for rows in (sc.rows["log_scale"], sc.rows["needle_disc"], sc.tiny):
        stress[rows] = True
    only3[stress[vis]] = 0
    for name, s in (("random slab", slab), ("opacity column", only3)):
        auto, ref, B, E = pose_reference_aa(case, s)
        assert float(((auto[:3] - ref).abs() / B).max()) < 1e-11   # the closed form on the folded slab IS the derivative
        got, again = run(s, True), run(s, True)
        assert torch.equal(got, again) and not got[3].any() and bool(torch.isfinite(got).all())
        r = pose_r(got, ref, B, E)
        r_classic = pose_r(run(s, False), ref, B, E)
        report(f"antialias_pose[{kind} deg {deg}, {name}]", r=r, r_of_the_classic_kernel=r_classic)
        print(f"antialias_pose[{kind} deg {deg}, {name}]: r = {r:.3g} (the classic kernel on the same slab: {r_classic:.3g})")
        assert r <= R_MAX, (name, r)
        if name == "opacity column":
            assert r_classic > 100 * R_MAX, r_classic   # the factor's term is what this case measures


# ---- frame ----------------------------------------------------------------------------------------------------------
PARAMS = ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")


def frame_inputs(grad=False):
    c = FRAME
    g, cam, T = make_scene(c["N"], c["W"], c["H"], 1, seed=c["seed"], device=DEV)
    g.opacity.add_(c["shift"])
    if grad:
        for k in PARAMS:
            getattr(g, k).requires_grad_(True)
    return g, cam, T, torch.full((3,), c["bg"], device=DEV)


@functools.lru_cache(maxsize=None)
def frame_reference():
    """the antialiased frame's own per-Gaussian outputs and complete lists; the float64 render reference fed the float64
    evaluation of opa_eff, the fp32 oracle fed the fp32 one; the float64 chain's parameter gradients with the abs sums
    carried through the stage, and the fp32 oracle chain's"""
    g, cam, T, bg = frame_inputs()
    W, H = FRAME["W"], FRAME["H"]
    d = DEFAULTS
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, d["near_thresh"],
                                 d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None, 0, antialiased=True)
    torch.cuda.synchronize()
    V = f.V
    cpu = lambda x: x.detach().cpu().contiguous()
    conic, y = cpu(f.conic[:V]), cpu(f.opacity_act[:V])
    gen = torch.Generator().manual_seed(FRAME["seed"] + 1)
    base = dict(W=W, H=H, V=V, uv=cpu(f.uv[:V]), conic=conic, coeff16=cpu(f.rgb_render[:V]).reshape(V, 3, 1),
                rays=torch.zeros(H, W, 3), grad_image=torch.randn(H, W, 3, generator=gen),
                bg=torch.full((3,), FRAME["bg"]), sorted_g=cpu(f.sorted_g).int(), ranges=cpu(f.ranges).int())
    opa64 = opacity_eff_fp64(conic.double(), y.double())
    opa32 = opacity_eff(conic, y, torch.float32)
    sc32 = SimpleNamespace(name="antialiased frame", opacity=opa32, **base)
    ref = R.render_fp64(base["uv"], opa64, R.scene_coeff(sc32, 1), conic, base["rays"], base["ranges"], base["sorted_g"],
                        base["bg"], W, H, R.FP32, base["grad_image"])
    ref.grad_image = (base["grad_image"].double() * (~ref.fragile)[:, :, None]).contiguous()
    orc = oracle_run(sc32, 1, torch.float32, ref.grad_image, exact=True)
    # accumulated opacity: the same walk with colour 1 on black
    ones = torch.full((V, 3, 1), 1.0 / SH_0)
    alpha_ref = R.render_fp64(base["uv"], opa64, ones, conic, base["rays"], base["ranges"], base["sorted_g"],
                              torch.zeros(3), W, H, R.FP32).image[:, :, 0]
    sc_a = SimpleNamespace(name="alpha", opacity=opa32, **dict(base, coeff16=ones.float(), bg=torch.zeros(3)))
    alpha_orc = oracle_run(sc_a, 1, torch.float32, torch.zeros(H, W, 3, dtype=torch.float64), exact=True)["image"][:, :, 0]
    # ---- the parameter gradients: float64 chain, carried abs sums, fp32 oracle chain ----
    cg = SimpleNamespace(**{k: (None if getattr(g, k) is None else getattr(g, k).detach().cpu()) for k in PARAMS})
    scene = SimpleNamespace(g=cg, cam=Camera(W, H, cam.K.cpu()), T=T.cpu(), W=W, H=H, near=d["near_thresh"],
                            far=d["far_thresh"], pad=d["cull_mask_padding"], mh=d["mh_dist"])
    st = oracle_stages(scene, torch.float32)
    assert st["V"] == V and torch.equal(st["conic"], conic)
    vis = torch.nonzero(st["keep"]).flatten()
    L = leaves64(cg)
    out = per_gaussian_fp64(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], scene.T, scene.cam.K,
                            W, H, scene.near, scene.far, scene.pad)
    yv = torch.cat([out["rgb_render"][vis], opacity_eff_fp64(out["conic"][vis], out["opacity_act"][vis]), out["uv"][vis],
                    out["conic"][vis]], dim=1)
    slab_of = lambda gr: torch.cat([gr["g_rgb"].reshape(V, 3), gr["g_opacity"], gr["g_uv"], gr["g_conic"]], dim=1).double()
    keys = [k for k in LEAVES if L[k] is not None]
    leaves = [L[k] for k in keys]
    grads = torch.autograd.grad(yv, leaves, grad_outputs=slab_of(ref.grad_walk), retain_graph=True, allow_unused=True)
    param_ref = {k: (torch.zeros_like(L[k]) if x is None else x) for k, x in zip(keys, grads)}
    a_slab = slab_of(ref.abs_walk)
    carried = {k: torch.zeros_like(L[k]) for k in keys}
    for j in range(9):
        go = torch.zeros_like(yv)
        go[:, j] = a_slab[:, j]
        for k, x in zip(keys, torch.autograd.grad(yv, leaves, grad_outputs=go, retain_graph=True, allow_unused=True)):
            if x is not None:
                carried[k] += x.detach().abs()
    orc_slab = torch.cat([orc["g_rgb"].reshape(V, 3), orc["g_opacity"], orc["g_uv"], orc["g_conic"]], dim=1).float()
    param_orc = oracle_vjp(scene, st, fold_slab(conic, y, orc_slab, torch.float32))
    return SimpleNamespace(ref=ref, orc=orc, alpha_ref=alpha_ref, alpha_orc=alpha_orc, param_ref=param_ref,
                           carried=carried, param_orc=param_orc, culled=st["culled"], V=V)


def image_r(got, want, orc, ok):
    n = int(ok.sum())
    return r_measure(got.double()[ok].reshape(n, -1), want[ok].reshape(n, -1), (orc.double() - want)[ok].reshape(n, -1))


def run_frame(g, cam, T, bg, fn=None, **kw):
    fn = fused.rasterize if fn is None else fn
    return fn(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS, **kw)


@pytest.mark.parametrize("mode", ["native", "python"])
def test_frame_against_the_fp64_chain(mode):
    if mode == "native" and fused.native() is None:
        pytest.skip("native frame module not built")
    fr = frame_reference()
    ref = fr.ref
    ok = ~ref.fragile
    g, cam, T, bg = frame_inputs(grad=True)
    prev = fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT
    fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT = mode == "native", False, False
    try:
        _hip.set_backward_mode("exact")
        image, mask, uv = run_frame(g, cam, T, bg, antialiased=True)
        image.backward(ref.grad_image.float().to(DEV))
        torch.cuda.synchronize()
    finally:
        _hip.set_backward_mode("compat")
        fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT = prev
    assert torch.equal(mask.cpu(), fr.culled)
    vals = {"fragile": float(ref.fragile.float().mean()), "V": fr.V}
    vals["r_image"] = image_r(image.detach().cpu(), ref.image, fr.orc["image"], ok)
    for k in fr.param_ref:
        got = getattr(g, k).grad.cpu()
        assert not got[fr.culled].any(), k
        vals[f"oracle_{k}"] = noise_measure(fr.param_orc[k], fr.param_ref[k], fr.carried[k])
        vals[f"kernel_{k}"] = noise_measure(got, fr.param_ref[k], fr.carried[k])
    report(f"antialias_frame[{mode}]", **vals)
    print(f"antialias_frame[{mode}]", {k: (round(v, 9) if isinstance(v, float) else v) for k, v in vals.items()})
    assert vals["fragile"] <= 0.05
    assert vals["r_image"] <= R_MAX, vals
    for k in fr.param_ref:
        assert vals[f"kernel_{k}"] <= vals[f"oracle_{k}"] + NOISE_MARGIN, (k, vals)
        assert getattr(g, k).grad.abs().max() > 0, k


def test_frame_orchestrations_policies_and_maps_agree():
    """native and Python orchestration, depth cut forced on and off: torch.equal images; antialiased=False is the
    default; rasterize_rgbd / rasterize_features give rasterize's image, and their alpha map is the reference's"""
    fr = frame_reference()
    g, cam, T, bg = frame_inputs()
    images = {}
    prev = fused.NATIVE, fused.DEPTH_CUT
    try:
        for native in (True, False):
            for cut in (False, True):
                if native and fused.native() is None:
                    continue
                fused.NATIVE, fused.DEPTH_CUT = native, cut
                before = fused.counters()["depth_cut_frames"]
                images[(native, cut)] = run_frame(g, cam, T, bg, antialiased=True)[0]
                assert fused.counters()["depth_cut_frames"] - before == int(cut), (native, cut)
    finally:
        fused.NATIVE, fused.DEPTH_CUT = prev
    first = images[(False, False)]
    for key, img in images.items():
        assert torch.equal(img, first), key
    classic = run_frame(g, cam, T, bg)[0]
    assert torch.equal(run_frame(g, cam, T, bg, antialiased=False)[0], classic)
    assert not torch.equal(classic, first)
    ok = ~fr.ref.fragile
    image_d, depth, alpha_d, _, _ = run_frame(g, cam, T, bg, fn=fused.rasterize_rgbd, antialiased=True)
    feat = torch.rand(g.xyz.shape[0], 3, device=DEV)
    image_f, fmap, alpha_f, _, _ = fused.rasterize_features(g, feat, T, cam, use_sh_precompute=True, background_rgb=bg,
                                                           antialiased=True, **DEFAULTS)
    assert torch.equal(image_d, first) and torch.equal(image_f, first) and torch.equal(alpha_d, alpha_f)
    r = image_r(alpha_d.cpu()[:, :, None], fr.alpha_ref[:, :, None], fr.alpha_orc[:, :, None], ok)
    report("antialias_frame[alpha map]", r=r)
    print(f"antialias_frame[alpha map]: r = {r:.3g}")
    assert r <= R_MAX, r
    assert torch.equal(run_frame(g, cam, T, bg, fn=fused.rasterize_rgbd, antialiased=False)[2],
                       run_frame(g, cam, T, bg, fn=fused.rasterize_rgbd)[2])


# ---- what the factor is for -----------------------------------------------------------------------------------------
def grid_scene(res):
    """an 11 x 11 grid of isotropic Gaussians 8 px apart at 96 x 96 (sigma 0.3 px there, opacity logit 0, random
    sub-pixel offsets, 7 px or more from the border: 10 x 8 + 2 x 8 = 96 leaves no room for the offsets), identity pose,
    fx = fy = W; rendered at res x res with K scaled by res / 96"""
    gen = torch.Generator().manual_seed(3)
    i, j = torch.meshgrid(torch.arange(11.0), torch.arange(11.0), indexing="ij")
    off = torch.rand(121, 2, generator=gen)
    u = 8.0 + 8.0 * i.reshape(-1) + off[:, 0]
    v = 8.0 + 8.0 * j.reshape(-1) + off[:, 1]
    z = 2.0
    xyz = torch.stack([(u - 48.0) * z / 96.0, (v - 48.0) * z / 96.0, torch.full_like(u, z)], dim=1)
    n = xyz.shape[0]
    scale = torch.full((n, 3), float(torch.log(torch.tensor(0.3 * z / 96.0))))
    quat = torch.zeros(n, 4)
    quat[:, 0] = 1.0
    k = res / 96.0
    K = torch.tensor([[96.0 * k, 0.0, 48.0 * k], [0.0, 96.0 * k, 48.0 * k], [0.0, 0.0, 1.0]])
    g = Gaussians(xyz.to(DEV), torch.full((n, 3), 1.0, device=DEV), torch.zeros(n, 1, device=DEV), scale.to(DEV),
                  quat.to(DEV), None)
    return g, Camera(res, res, K.to(DEV)), torch.eye(4, device=DEV)


def test_minification_keeps_the_deposited_light():
    R_ = {}
    for aa in (True, False):
        total = {}
        for res in (96, 384):
            g, cam, T = grid_scene(res)
            _, _, alpha, mask, _ = fused.rasterize_rgbd(g, T, cam, use_sh_precompute=True,
                                                        background_rgb=torch.zeros(3, device=DEV), antialiased=aa,
                                                        **DEFAULTS)
            assert not mask.any()
            total[res] = float(alpha.double().sum())
        R_[aa] = 16.0 * total[96] / total[384]
    report("antialias_minification", antialiased=R_[True], classic=R_[False])
    print(f"antialias_minification: R = {R_[True]:.4f} antialiased, {R_[False]:.4f} classic")
    assert 0.9 <= R_[True] <= 1.1, R_
    assert R_[False] > 2.5, R_


def test_training_smoke():
    N, W, H = 3000, 64, 48
    g, cam, T = make_scene(N, W, H, 1, seed=11, device=DEV)
    bg = torch.full((3,), 0.5, device=DEV)
    with torch.no_grad():
        target = run_frame(g, cam, T, bg, antialiased=True)[0].clone()
    gen = torch.Generator().manual_seed(12)
    noise = lambda x, s: x + s * torch.randn(x.shape, generator=gen).to(DEV)
    params = dict(xyz=noise(g.xyz, 0.01), rgb=noise(g.rgb, 0.2), opacity=noise(g.opacity, 0.5), scale=noise(g.scale, 0.1),
                  quaternion=noise(g.quaternion, 0.05), sh=noise(g.sh, 0.02))
    for v in params.values():
        v.requires_grad_(True)
    gp = Gaussians(params["xyz"], params["rgb"], params["opacity"], params["scale"], params["quaternion"], params["sh"])
    lrs = dict(xyz=2e-4, rgb=1e-2, opacity=2e-2, scale=5e-3, quaternion=1e-3, sh=5e-4)
    opt = torch.optim.Adam([{"params": [params[k]], "lr": lrs[k]} for k in params])
    losses = []
    for _ in range(40):
        opt.zero_grad(set_to_none=True)
        image = run_frame(gp, cam, T, bg, antialiased=True)[0]
        loss = (image - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        final = float((run_frame(gp, cam, T, bg, antialiased=True)[0] - target).abs().mean())
    report("antialias_training_smoke", initial=losses[0], final=final)
    print(f"antialias_training_smoke: loss {losses[0]:.5f} -> {final:.5f}")
    for k, v in params.items():
        assert bool(torch.isfinite(v).all()), k
    assert final < losses[0]


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_frame_alone():
    g, cam, T = make_scene(3000, 64, 48, 1, seed=11, device=DEV)
    bg = torch.full((3,), 0.5, device=DEV)
    before = run_frame(g, cam, T, bg)[0].clone()
    before_aa = run_frame(g, cam, T, bg, antialiased=True)[0].clone()
    # (any plan object: the refusal comes before the plan is looked at)
    refused = [dict(adam_plan=object()), dict(tile_rows=(0, 2)), dict(return_aux=True), dict(grad_sync=lambda t: t),
               dict(slab_sync=lambda t: None), dict(frame_hook=lambda d: None)]
    for kw in refused:
        for fn in (fused.rasterize, fused.rasterize_rgbd):
            with pytest.raises(RuntimeError, match="antialiased|rasterize_rgbd"):
                run_frame(g, cam, T, bg, fn=fn, antialiased=True, **kw)
    with pytest.raises(RuntimeError, match="per-pixel SH"):
        fused.rasterize(g, T, cam, use_sh_precompute=False, background_rgb=bg, antialiased=True, **DEFAULTS)
    g64 = Gaussians(*[None if x is None else x.detach().double() for x in (g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, g.sh)])
    with pytest.raises(RuntimeError, match="float32 tensors on the GPU"):
        fused.rasterize(g64, T.double(), Camera(64, 48, cam.K.double()), use_sh_precompute=True,
                        background_rgb=bg.double(), antialiased=True, **DEFAULTS)
    cpu = Gaussians(*[None if x is None else x.detach().cpu() for x in (g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, g.sh)])
    with pytest.raises(RuntimeError, match="float32 tensors on the GPU"):
        fused.rasterize(cpu, T.cpu(), Camera(64, 48, cam.K.cpu()), use_sh_precompute=True, background_rgb=bg.cpu(),
                        antialiased=True, **DEFAULTS)
    with pytest.raises(RuntimeError, match="tile_rows"):
        fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, 64, 48, 0.3, 500.0, 100,
                                 3.0, (0, 2), 0, antialiased=True)
    with torch.no_grad():
        assert torch.equal(run_frame(g, cam, T, bg)[0], before)
        assert torch.equal(run_frame(g, cam, T, bg, antialiased=True)[0], before_aa)
