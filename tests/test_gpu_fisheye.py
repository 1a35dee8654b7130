"""fused.rasterize(camera_model="fisheye") / GS_RASTER_FISHEYE (ABI 19): the per-Gaussian kernels' fisheye
instantiations at the stage level, the pose gradient, a known-answer scene, the frame through both orchestrations, a
short training run and the refusals.

The oracle has no fisheye model.  Stage measures: ref64.r_measure against the float64 evaluation of
tests/fisheye_ref.py with env = |its float32 evaluation - float64|, bound R_MAX = 8
(tests/test_gpu_general_cameras.py).  Rows are left out only where the float64 u or v lies within 1e-3 px of a frustum
edge or z within 1e-6 (relative) of near or far (fisheye_ref.left_out; under 0.5 % of the visible rows, which
tests/test_fisheye_ref.py holds for the reference alone); on every other row the culling mask must be the float64
decision.  Mode 3 (antialiased + fisheye): tests/antialias_ref.py on the fisheye conic, rows whose det_0 > 0 decision
differs between the precisions left out as in tests/test_gpu_antialias.py.  Pose: the measure and bound of
tests/test_gpu_pose_grad.py with the closed form of fisheye_ref.pose_terms_fisheye, held to autograd first.

Scenes: general_camera_scene(130 + deg, 6000) for landscape / 3, odd / 0, one_tile_wide / 2 with their stress rows, and
fisheye_ref.wide_scene (theta up to 85 degrees, four rows at exactly x = y = 0).

Measured on an MI355X (every case prints its figures and leaves them in the parity report):
  forward   uv 0.85 .. 1.02, conic and packed a, b, c 0.26 .. 2.36, cut and non-cut equal bits; no row left out on any
            scene; wide: 3 469 of 6 000 visible, the four on-axis rows exactly on the principal point
  mode 3    opacity against antialias_ref on the kernel's conic 1.00 (odd) / 0.62 (wide); against the float64 chain the
            ratio to the float32 chain's envelope is 123 / 1.15 (printed), the error 0.49 / 0.002 of what the conic's
            admissible error carried through the factor allows (asserted <= 1); the 11 rows of odd over 8 in the ratio
            have det_0 / (a0 c0) <= 0.006
  backward  whole set 0.19 .. 2.01, owner slice 0.16 .. 3.00 (odd, xyz)
  pose      2.02 / 0.97 / 0.74 / 0.06 (wide); closed form against autograd 3e-16 .. 1e-12 of B; the pinhole kernel on
            the same slab 1.4e6 and more
  known answer  uv r 0.19, 32 of 32 local maxima on their pixel
  frame     native against Python gradients at most 1e-7 of the largest element (the atomics' order: run to run);
            FRAME against the float64 chain, native and Python alike: r_image 0.81, parameter gradients kernel
            4.7e-6 .. 3.08e-5 against the fp32 chain's 4.8e-6 .. 3.06e-5 (at most 1.4e-7 above it)
  training  L1 0.0264 -> 0.0030 in 40 steps"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.splat_py.structs import Camera, Gaussians
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

from . import fisheye_ref as F
from . import render_ref64 as R
from .antialias_ref import aa_terms, opacity_eff, opacity_eff_fp64
from .helpers import report
from .pose_terms import pose_r
from .ref64 import SH_0, r_measure, random_slab, to_device
from .test_gpu_antialias import raw_backward, raw_forward
from .test_gpu_render_ref64 import FRAME, NOISE_MARGIN, noise_measure
from .test_render_ref64 import oracle_run

pytestmark = pytest.mark.gpu
DEV = "cuda"
R_MAX = 8.0
NAMES = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
CLASSIC, AA, FISH = 0, 1, 2
LEFT_OUT_MAX = 0.005


def p(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def stage_case(name):
    """scene, its float64 and float32 fisheye stages, the rows left out"""
    sc = F.scene(name)
    ref, f32 = F.stage(sc, torch.float64), F.stage(sc, torch.float32)
    return SimpleNamespace(sc=sc, ref=ref, f32=f32, out=F.left_out(ref, sc), name=name)


def stage_forward(sc, model, aa=False, cut=False):
    g, cam, T = to_device(sc, DEV)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, sc.near,
                                 sc.far, sc.pad, sc.mh, None, 0 if not cut else _hip.GS_SORT_PREFIX, depth_cut=cut,
                                 antialiased=aa, camera_model=model)
    torch.cuda.synchronize()
    V = f.V
    c = lambda x: x[:V].detach().cpu()
    got = dict(uv=c(f.uv), xyz_cam=c(f.xyz_cam), conic=c(f.conic), opacity_act=c(f.opacity_act), rgb_render=c(f.rgb_render),
               packed=c(f.packed), vis_idx=c(f.vis_idx), culling_mask=f.culling_mask.cpu(), rank=f.rank.cpu())
    if cut:
        got["bin_rec"] = f.cut.bin_rec.view(-1, 8)[:V].cpu()
    return f, got, (g, cam, T)


def check(tag, rs):
    report(tag, **rs)
    print(tag, {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rs.items()})
    for k, v in rs.items():
        if k.startswith("r_"):
            assert v <= R_MAX, (tag, k, v)


def check_mask_and_ranks(case, got):
    """the culling mask is the float64 decision outside the left-out rows; rank, vis_idx and V follow the mask.
    -> (visible Gaussian indices, which of them enter the comparisons)"""
    mask, rank, vis = got["culling_mask"], got["rank"].long(), got["vis_idx"].long()
    keep = ~case.out
    assert torch.equal(mask[keep], case.ref["culled"][keep])
    V = int((~mask).sum())
    assert vis.shape[0] == V and torch.equal(vis, torch.nonzero(~mask).flatten())
    assert torch.equal(rank[~mask], torch.arange(V)) and bool((rank[mask] == -1).all())
    n_out = int((case.out & ~mask).sum())
    assert n_out < LEFT_OUT_MAX * V, (n_out, V)
    return vis, ~case.out[vis] & ~case.ref["culled"][vis], n_out


# ---- 1. forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.SCENES)
def test_forward(name):
    assert (_hip.GS_RASTER_CLASSIC, _hip.GS_RASTER_ANTIALIASED, _hip.GS_RASTER_FISHEYE) == (CLASSIC, AA, FISH)
    case = stage_case(name)
    sc, ref, f32 = case.sc, case.ref, case.f32
    ntx, nty = (sc.W + 15) // 16, (sc.H + 15) // 16
    cut_ok = bool(_hip.lib().gs_cut_supported(ntx, 0, nty, sc.g.xyz.shape[0]))
    _, pin, _ = stage_forward(sc, "pinhole")
    first = None
    for cut in (False, True):
        if cut and not cut_ok:   # the per-Gaussian entry point's cut form alone
            status, got, _ = raw_forward(sc, *to_device(sc, DEV), FISH, cut=True)
            assert status == 0
        else:
            _, got, _ = stage_forward(sc, "fisheye", cut=cut)
        vis, sel, n_out = check_mask_and_ranks(case, got)
        gi = vis[sel]
        rs = dict(V=int(vis.shape[0]), left_out=n_out)
        for k in ("uv", "conic"):
            rs["r_" + k] = r_measure(got[k][sel], ref[k][gi], f32[k][gi].double() - ref[k][gi])
        pk = got["packed"][sel]
        rs["r_packed_uv"] = r_measure(pk[:, 0:2], ref["uv"][gi], f32["uv"][gi].double() - ref["uv"][gi])
        rs["r_packed_abc"] = r_measure(pk[:, 4:7], ref["packed_abc"][gi], f32["packed_abc"][gi].double() - ref["packed_abc"][gi])
        if cut:
            br = got["bin_rec"]
            assert torch.equal(br[:, 0:2], got["uv"]) and torch.equal(br[:, 2:5], got["conic"])
            assert torch.equal(br[:, 5], got["xyz_cam"][:, 2])
        for k in ("uv", "xyz_cam", "conic", "opacity_act", "rgb_render", "packed"):
            assert bool(torch.isfinite(got[k]).all()), k
        # what the model leaves alone: the bits of the pinhole run on the rows visible in both
        both = ~got["culling_mask"] & ~pin["culling_mask"]
        rf, rp = got["rank"].long()[both], pin["rank"].long()[both]
        assert int(both.sum()) > 500
        for k in ("xyz_cam", "opacity_act", "rgb_render"):
            assert torch.equal(got[k][rf], pin[k][rp]), (cut, k)
        # the optical-axis rows: finite, inside the comparisons, uv on the principal point
        axis = sc.rows["optical_axis"]
        on = axis[~got["culling_mask"][axis]]
        assert on.numel() > 0 and bool(sel[got["rank"].long()[on]].all())
        if name == "wide":
            assert on.numel() == 4
            assert torch.equal(got["uv"][got["rank"].long()[on]], sc.cam.K[:2, 2].expand(4, 2))
        check(f"fisheye_forward[{name} cut {cut}]", rs)
        if first is None:
            first = got
        else:
            for k in first:
                assert torch.equal(first[k], got[k]), k


@pytest.mark.parametrize("name", ["odd", "wide"])
def test_forward_modes(name):
    """mode 3: the record's opacity is the antialiased one of the fisheye conic, everything else mode 2's bits; modes 0
    and 1 through the _mode entry are the classic and the antialiased call; modes 4 and 7 return GS_EINVAL and write
    nothing"""
    case = stage_case(name)
    sc, ref, f32 = case.sc, case.ref, case.f32
    _, fish, dev = stage_forward(sc, "fisheye")
    _, both, _ = stage_forward(sc, "fisheye", aa=True)
    for k in fish:
        if k != "packed":
            assert torch.equal(both[k], fish[k]), k
    cols = [0, 1] + list(range(4, 12))
    assert torch.equal(both["packed"][:, cols], fish["packed"][:, cols])
    vis, sel, _ = check_mask_and_ranks(case, both)
    # tests/antialias_ref.py applied to the fisheye conic the kernel wrote (as tests/test_gpu_antialias.py applies it to
    # the conic bits both sides share): float64 and fp32 evaluation of the header's expressions on those bits
    conic, y = both["conic"], both["opacity_act"]
    t32, t64 = aa_terms(conic, torch.float32), aa_terms(conic.double(), torch.float64)
    det_differs = (t32["det_0"] > 0) != (t64["det_0"] > 0)
    assert int(det_differs.sum()) < LEFT_OUT_MAX * vis.shape[0]
    ok = ~det_differs
    opa64 = opacity_eff_fp64(conic.double(), y.double())
    own = opacity_eff(conic, y, torch.float32)
    r = r_measure(both["packed"][:, 3:4][ok], opa64[ok], own[ok].double() - opa64[ok])
    # The same column against the float64 CHAIN (float64 conic -> float64 factor, envelope from the float32 chain).  The
    # ratio to that envelope is printed, not bounded: one fp32 sample of an ill-conditioned quantity does not bound
    # another.  What is bounded instead settles whose fault an excess is: the kernel's conic is within R_MAX of its own
    # envelope (test_forward asserts it), so its factor may differ from the float64 chain's by that admissible conic
    # error carried through the factor, to first order
    #     |d comp| / comp <= E / det_0 (1 - E / det_0)^-1 + E / det_d,   E = c0 da0 + a0 dc0 + |b| dconic1 + 3 2^-24 (a0 c0 + b b)
    # (the last term: the fp32 evaluation of det_0 itself), plus the product's own rounding; where E reaches det_0 / 2
    # the factor is not determined at fp32 at all and anything in [0, y] is admissible.
    ok2 = sel & ~det_differs
    c64, y64 = ref["conic"][vis], ref["opacity_act"][vis]
    chain64 = opacity_eff_fp64(c64, y64)
    chain32 = opacity_eff(f32["conic"][vis], f32["opacity_act"][vis], torch.float32)
    chain = r_measure(both["packed"][:, 3:4][ok2], chain64[ok2], chain32[ok2].double() - chain64[ok2])
    env_c = (f32["conic"][vis].double() - c64).abs()
    d_conic = R_MAX * (env_c + 2.0 ** -22 * c64.abs() + 1e-7 * c64[sel].abs().max(dim=0, keepdim=True).values)
    t = aa_terms(c64, torch.float64)
    E = (t["c0"].abs() * d_conic[:, 0] + t["a0"].abs() * d_conic[:, 2] + t["b"].abs() * d_conic[:, 1]
         + 3 * 2.0 ** -24 * (t["a0"] * t["c0"] + t["b"] * t["b"]).abs())
    rel = E / t["det_0"].clamp(min=1e-300)
    first_order = t["comp"] * (rel / (1 - rel).clamp(min=0.5) + E / t["det_d"])
    admissible = torch.where(rel < 0.5, y64[:, 0] * first_order, y64[:, 0]) + 8 * 2.0 ** -22 * y64[:, 0]
    err = (both["packed"][:, 3].double() - chain64[:, 0]).abs()
    over_admissible = float((err[ok2] / admissible[ok2]).max())
    # and where the chain ratio exceeds the bound, det_0 has cancelled: det_0 / (a0 c0) of those rows
    row_r = err / ((chain32.double() - chain64).abs()[:, 0] + 2.0 ** -22 * chain64[:, 0].abs()
                   + 1e-7 * chain64[ok2].abs().max())
    excess = ok2 & (row_r > R_MAX)
    kappa = (t["det_0"] / (t["a0"] * t["c0"]))
    check(f"fisheye_forward_modes[{name}]", dict(r_opacity_mode3=r, det_left_out=int(det_differs.sum()),
                                                equal_to_fp32_evaluation=float((both["packed"][:, 3:4] == own).float().mean()),
                                                against_the_float64_chain=chain, chain_error_over_admissible=over_admissible,
                                                rows_over_the_chain_bound=int(excess.sum()),
                                                their_largest_det0_over_a0c0=float(kappa[excess].max()) if bool(excess.any()) else 0.0))
    assert over_admissible <= 1.0, over_admissible
    assert bool((both["packed"][:, 3] <= fish["packed"][:, 3]).all())
    # modes 0 and 1
    _, pin, _ = stage_forward(sc, "pinhole")
    _, pin_aa, _ = stage_forward(sc, "pinhole", aa=True)
    for mode, want in ((CLASSIC, pin), (AA, pin_aa)):
        status, got, _ = raw_forward(sc, *dev, mode)
        assert status == 0
        for k in got:
            assert torch.equal(got[k], want[k]), (mode, k)
    status, old, _ = raw_forward(sc, *dev, None)   # gs_preprocess_forward_cut without the cut: today's entry
    assert status == 0 and all(torch.equal(old[k], pin[k]) for k in old)
    status, got, _ = raw_forward(sc, *dev, FISH)
    assert status == 0 and all(torch.equal(got[k], fish[k]) for k in got)
    for mode in (4, 7):
        status, got, o = raw_forward(sc, *dev, mode)
        assert status == _hip.GS_EINVAL and got is None and b"raster_mode" in _hip.lib().gs_last_error()
        for t, fill in ((o.packed, 7.0), (o.uv, 7.0), (o.conic, 7.0), (o.opa, 7.0), (o.rank, -3), (o.vis, -3), (o.ws, -3)):
            assert bool((t == fill).all())


# ---- 2. backward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.SCENES)
def test_backward(name):
    case = stage_case(name)
    sc = case.sc
    N = sc.g.xyz.shape[0]
    f, got_f, (g, cam, T) = stage_forward(sc, "fisheye")
    vis, _, _ = check_mask_and_ranks(case, got_f)
    V = f.V
    slab = random_slab(V, 5)
    ref_g = F.stage(sc, torch.float64, slab, vis)["grad"]
    env_g = F.stage(sc, torch.float32, slab, vis)["grad"]
    slab_d = slab.to(DEV).contiguous()
    cpu = lambda out: {k: (None if x is None else x.cpu()) for k, x in zip(NAMES, out)}
    culled = got_f["culling_mask"]
    ok = ~case.out

    def measure(got, i0=0, i1=N):
        rs = {}
        for k in got:
            if got[k] is None:
                continue
            assert not got[k][culled[i0:i1]].any(), k   # culled rows: exactly zero
            assert bool(torch.isfinite(got[k]).all()), k
            r, e, o = ref_g[k][i0:i1], env_g[k][i0:i1].double(), ok[i0:i1]
            rs["r_" + k] = r_measure(got[k][o], r[o], e[o] - r[o])
        return rs

    run = lambda s, **kw: fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, s, **kw)
    whole = cpu(run(slab_d, camera_model="fisheye"))
    check(f"fisheye_backward[{name}] whole set", measure(whole))
    i0, i1 = 256, 1792
    v_base = int((~culled[:i0]).sum())
    part = cpu(run(slab_d[v_base:].contiguous(), v_base=v_base, i0=i0, i1=i1, camera_model="fisheye"))
    check(f"fisheye_backward[{name}] owner slice", measure(part, i0, i1))
    for k in part:
        if part[k] is not None:
            assert torch.equal(part[k], whole[k][i0:i1]), k
    # the optical-axis rows take part
    on = sc.rows["optical_axis"]
    on = on[~culled[on]]
    assert on.numel() > 0 and bool(ok[on].all()) and bool(whole["xyz"][on].any())
    # nothing model-dependent left: the pinhole backward's bits
    flat = slab_d.clone()
    flat[:, 4:] = 0
    a, b = run(flat, camera_model="fisheye"), run(flat)
    for k, x, y in zip(NAMES, a, b):
        assert (x is None and y is None) or torch.equal(x, y), k
    # and with them the model is in it
    c, d = run(slab_d, camera_model="fisheye"), run(slab_d)
    assert not torch.equal(c[0], d[0])
    # antialiased + fisheye: finite, and the fold's term reaches the scale through the fisheye conic
    only3 = torch.zeros_like(slab_d)
    only3[:, 3] = slab_d[:, 3]
    e = run(only3, camera_model="fisheye", antialiased=True)
    assert bool(e[2].any()) and all(x is None or bool(torch.isfinite(x).all()) for x in e)
    # the entry point: modes 4 and 7 are refused and write nothing
    for mode in (4, 7):
        status, untouched = raw_backward("gs_preprocess_backward_mode", g, cam, T, f, slab_d, f.n_sh, [mode])
        assert status == _hip.GS_EINVAL and b"raster_mode" in _hip.lib().gs_last_error()
        assert all(x is None or bool((x == 7.0).all()) for x in untouched)
    status, new = raw_backward("gs_preprocess_backward_mode", g, cam, T, f, slab_d, f.n_sh, [FISH])
    assert status == 0 and all(x is None or torch.equal(x.cpu(), whole[k]) for k, x in zip(NAMES, new))


# ---- 3. pose ----------------------------------------------------------------------------------------------------------
def pose_reference(case, vis, slab):
    """(float64 autograd's dL/dT through the fisheye stage; sum t64, B, E of the closed form's per-Gaussian terms)"""
    sc, g = case.sc, case.sc.g
    L = F.leaves(g, torch.float64, requires_grad=False)
    T64 = sc.T.double().clone().requires_grad_(True)
    out = F.per_gaussian_fisheye(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], T64, sc.cam.K,
                                 sc.W, sc.H, sc.near, sc.far, sc.pad)
    y = torch.cat([out["uv"][vis], out["conic"][vis]], dim=1)
    (auto,) = torch.autograd.grad(y, T64, grad_outputs=slab[:, 4:].double())
    rows = (g.xyz[vis], g.quaternion[vis], g.scale[vis], sc.T, sc.cam.K)
    t64 = F.pose_terms_fisheye(*rows, slab, torch.float64)
    t32 = F.pose_terms_fisheye(*rows, slab, torch.float32).double()
    return auto, t64.sum(0), t64.abs().sum(0), (t32 - t64).abs().sum(0)


@pytest.mark.parametrize("name", F.SCENES)
def test_pose(name):
    case = stage_case(name)
    sc = case.sc
    f, got_f, (g, cam, T) = stage_forward(sc, "fisheye")
    vis, sel, _ = check_mask_and_ranks(case, got_f)
    slab = random_slab(f.V, 17)
    slab[~sel] = 0   # left-out rows carry nothing
    auto, ref, B, E = pose_reference(case, vis, slab)
    closed_vs_autograd = float(((auto[:3] - ref).abs() / B).max())
    assert closed_vs_autograd < 1e-11, closed_vs_autograd   # the closed form IS the derivative
    run = lambda model: fused.pose_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab.to(DEV).contiguous(),
                                            camera_model=model)
    got, again = run("fisheye"), run("fisheye")
    assert torch.equal(got, again) and not got[3].any() and bool(torch.isfinite(got).all())
    r, r_pin = pose_r(got, ref, B, E), pose_r(run("pinhole"), ref, B, E)
    check(f"fisheye_pose[{name}]", dict(r_pose=r, the_pinhole_kernel=r_pin, closed_form_vs_autograd=closed_vs_autograd))
    if name == "wide":
        assert r_pin > 100 * R_MAX, r_pin
    lib = _hip.lib()
    grad = torch.full((4, 4), 7.0, device=DEV)
    ws = torch.empty(lib.gs_pose_workspace_floats(sc.g.xyz.shape[0]), device=DEV)
    for mode in (4, 7):
        status = lib.gs_pose_backward_mode(p(g.xyz), p(g.quaternion), p(g.scale), p(T), p(cam.K), p(f.rank),
                                           p(f.opacity_act), p(slab.to(DEV)), 0, sc.g.xyz.shape[0], p(ws), p(grad), mode,
                                           _hip.current_stream())
        torch.cuda.synchronize()
        assert status == _hip.GS_EINVAL and bool((grad == 7.0).all())


# ---- 4. known answer --------------------------------------------------------------------------------------------------
def known_answer_scene():
    """tiny isotropic Gaussians 5 away on directions (theta, phi), theta 10 .. 80 degrees, chosen so that each projects
    (0.2, -0.15) px off an integer pixel position -- nearest to that pixel by a wide margin, and not on it: the render
    gives a splat no weight at a pixel it sits on exactly (mh == 0, the reference's test); identity pose, 256 x 256,
    fx = 88, fy = 80"""
    W = H = 256
    fx, fy, cx, cy = 88.0, 80.0, 128.0, 120.0
    pts = []
    for i, deg in enumerate(range(10, 81, 10)):
        for j in range(4):
            th, ph = math.radians(deg), math.radians(90.0 * j + 11.0 * i)
            pts.append((round(cx + fx * th * math.cos(ph)), round(cy + fy * th * math.sin(ph))))
    px = torch.tensor(pts, dtype=torch.float64) + torch.tensor([0.2, -0.15], dtype=torch.float64)
    du, dv = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
    theta, phi = torch.sqrt(du * du + dv * dv), torch.atan2(dv, du)
    rho = 5.0
    xyz = torch.stack([rho * torch.sin(theta) * torch.cos(phi), rho * torch.sin(theta) * torch.sin(phi),
                       rho * torch.cos(theta)], dim=1)
    n = xyz.shape[0]
    quat = torch.zeros(n, 4)
    quat[:, 0] = 1.0
    g = Gaussians(xyz.float().to(DEV), torch.full((n, 3), 1.0 / SH_0, device=DEV), torch.full((n, 1), 2.0, device=DEV),
                  torch.full((n, 3), math.log(1.2 * rho / fx), device=DEV), quat.to(DEV), None)
    K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    return g, Camera(W, H, K.to(DEV)), torch.eye(4, device=DEV), px, theta, phi, (fx, fy, cx, cy)


def test_known_answer():
    g, cam, T, px, theta, phi, (fx, fy, cx, cy) = known_answer_scene()
    assert float(theta.max()) > math.radians(78.0)
    bg = torch.zeros(3, device=DEV)
    image, mask, uv = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, camera_model="fisheye",
                                      **DEFAULTS)
    assert not mask.any()
    want = torch.stack([cx + fx * theta * torch.cos(phi), cy + fy * theta * torch.sin(phi)], dim=1)
    assert float((want - px).abs().max()) < 1e-9
    # the forward bound with the fp32 evaluation of the same expression as envelope
    env = torch.stack([(cx + fx * theta.float() * torch.cos(phi.float())).double(),
                       (cy + fy * theta.float() * torch.sin(phi.float())).double()], dim=1) - want
    # (the positions themselves were rounded to fp32: their share, |d uv / d c| * 2^-24 |c|, joins the envelope)
    env = env.abs() + 2.0 ** -24 * 4 * max(fx, fy)   # |c| = 5, |d uv / d c| <= ~fx / 5 per component, three components
    r = r_measure(uv.cpu(), want, env)
    lum = image[:, :, 0].cpu()
    on_pixel = 0
    for k in range(px.shape[0]):
        ix, iy = round(float(px[k, 0])), round(float(px[k, 1]))
        assert 3 <= ix < 256 - 3 and 3 <= iy < 256 - 3
        win = lum[iy - 3:iy + 4, ix - 3:ix + 4]
        on_pixel += int(int(win.argmax()) == 3 * 7 + 3 and float(win.max()) > 0.2)
    check("fisheye_known_answer", dict(r_uv=r, local_maxima_on_their_pixel=on_pixel, of=int(px.shape[0])))
    assert on_pixel == px.shape[0]
    # the pinhole model on the same scene culls exactly the rows whose tan(theta) carries them beyond the pad
    _, mask_pin, _ = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, camera_model="pinhole",
                                     **DEFAULTS)
    u = cx + fx * torch.tan(theta) * torch.cos(phi)
    v = cy + fy * torch.tan(theta) * torch.sin(phi)
    pad = DEFAULTS["cull_mask_padding"]
    beyond = (u < -pad) | (u > 256 + pad) | (v < -pad) | (v > 256 + pad)
    assert 4 <= int(beyond.sum()) < px.shape[0] and torch.equal(mask_pin.cpu(), beyond)


# ---- 5. frame ---------------------------------------------------------------------------------------------------------
def small_frame(grad=False):
    g, cam, T = make_scene(3000, 64, 48, 1, seed=11, device=DEV)
    if grad:
        for k in NAMES:
            getattr(g, k).requires_grad_(True)
    return g, cam, T, torch.full((3,), 0.5, device=DEV)


def run_frame(g, cam, T, bg, fn=None, **kw):
    fn = fused.rasterize if fn is None else fn
    return fn(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS, **kw)


def test_frame_orchestrations_policies_and_maps_agree():
    g, cam, T, bg = small_frame()
    images = {}
    prev = fused.NATIVE, fused.DEPTH_CUT
    try:
        for native in (True, False):
            for cut in (False, True):
                if native and fused.native() is None:
                    continue
                fused.NATIVE, fused.DEPTH_CUT = native, cut
                before = fused.counters()["depth_cut_frames"]
                images[(native, cut)] = run_frame(g, cam, T, bg, camera_model="fisheye")
                assert fused.counters()["depth_cut_frames"] - before == int(cut), (native, cut)
    finally:
        fused.NATIVE, fused.DEPTH_CUT = prev
    assert (True, False) in images, "native frame module not built"
    first, mask, uv = images[(False, False)]
    for key, (img, m, u) in images.items():
        assert torch.equal(img, first) and torch.equal(m, mask) and torch.equal(u, uv), key
    plain = run_frame(g, cam, T, bg)
    named = run_frame(g, cam, T, bg, camera_model="pinhole")
    assert all(torch.equal(a, b) for a, b in zip(plain, named)) and not torch.equal(plain[0], first)
    # the frame is the render of its own per-Gaussian stage: uv is the stage's
    d = DEFAULTS
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, 64, 48, d["near_thresh"],
                                 d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None, 0, camera_model="fisheye")
    assert torch.equal(f.uv[:f.V], uv) and torch.equal(f.culling_mask, mask)
    kw = dict(camera_model="fisheye")
    image_d, depth, alpha_d, mask_d, uv_d = run_frame(g, cam, T, bg, fn=fused.rasterize_rgbd, **kw)
    image_t = run_frame(g, cam, T, bg, fn=fused.rasterize_distortion, **kw)[0]
    feat = torch.rand(g.xyz.shape[0], 3, device=DEV)
    image_f, _, alpha_f, _, _ = fused.rasterize_features(g, feat, T, cam, use_sh_precompute=True, background_rgb=bg,
                                                        **DEFAULTS, **kw)
    image_c, stats, mask_c = run_frame(g, cam, T, bg, fn=fused.rasterize_contributions, **kw)
    for img in (image_d, image_t, image_f, image_c):
        assert torch.equal(img, first)
    assert torch.equal(alpha_d, alpha_f) and torch.equal(mask_d, mask) and torch.equal(uv_d, uv) and torch.equal(mask_c, mask)
    assert bool((stats.pixel_count > 0).any()) and not bool(stats.pixel_count[mask].any())
    # absgrad and antialiased combine
    image_a, _, uv_a, uv_abs = run_frame(g, cam, T, bg, absgrad=True, **kw)
    assert torch.equal(image_a, first) and torch.equal(uv_a, uv) and uv_abs.shape == uv.shape
    image_aa = run_frame(g, cam, T, bg, antialiased=True, **kw)[0]
    assert bool(torch.isfinite(image_aa).all()) and not torch.equal(image_aa, first)
    # rasterize_rgbd's depth has a gradient that reaches xyz
    g2, cam, T, bg = small_frame(grad=True)
    depth2 = run_frame(g2, cam, T, bg, fn=fused.rasterize_rgbd, **kw)[1]
    assert torch.equal(depth2, depth)
    depth2.sum().backward()
    assert bool(torch.isfinite(g2.xyz.grad).all()) and bool(g2.xyz.grad[~mask].any()) and not bool(g2.xyz.grad[mask].any())


def test_frame_gradients_native_and_python_agree():
    """the two orchestrations against each other only (the float64 yardstick is test_frame_against_the_fp64_chain's):
    the same image bit for bit, every parameter gradient and the pose's within summation noise of the other's"""
    prev = fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT
    grads, images = {}, {}
    gen = torch.Generator().manual_seed(3)
    gi = torch.randn(48, 64, 3, generator=gen).to(DEV)
    try:
        for native in (True, False):
            fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT = native, False, False
            g, cam, T, bg = small_frame(grad=True)
            T = T.clone().requires_grad_(True)
            image = run_frame(g, cam, T, bg, camera_model="fisheye")[0]
            image.backward(gi)
            torch.cuda.synchronize()
            images[native] = image.detach()
            grads[native] = {k: getattr(g, k).grad.clone() for k in NAMES} | {"pose": T.grad.clone()}
    finally:
        fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT = prev
    assert torch.equal(images[True], images[False])
    worst = {}
    for k in grads[True]:
        a, b = grads[True][k].double(), grads[False][k].double()
        assert bool(torch.isfinite(a).all()) and bool(a.any()), k
        # (the two orchestrations' render backwards add their atomics in different orders: summation noise only)
        worst["d_" + k] = float((a - b).abs().max() / b.abs().max())
        assert worst["d_" + k] < 1e-4, (k, worst)
    check("fisheye_frame[native vs python gradients]", worst)


# ---- 5b. the frame against the float64 chain ---------------------------------------------------------------------------
def frame_inputs(grad=False):
    c = FRAME
    g, cam, T = make_scene(c["N"], c["W"], c["H"], 1, seed=c["seed"], device=DEV)
    g.opacity.add_(c["shift"])
    if grad:
        for k in NAMES:
            getattr(g, k).requires_grad_(True)
    return g, cam, T, torch.full((3,), c["bg"], device=DEV)


@functools.lru_cache(maxsize=None)
def frame_reference():
    """the fisheye frame's own per-Gaussian outputs and complete lists; the float64 render reference and the fp32 render
    oracle fed them; the float64 chain's parameter gradients (float64 fisheye stage under autograd, fed the float64
    render gradients) with the abs sums carried through the stage, and the fp32 chain's (float32 evaluation of
    tests/fisheye_ref.py fed the fp32 oracle's render gradients: the oracle has no fisheye stage)"""
    g, cam, T, bg = frame_inputs()
    W, H = FRAME["W"], FRAME["H"]
    d = DEFAULTS
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, d["near_thresh"],
                                 d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None, 0, camera_model="fisheye")
    torch.cuda.synchronize()
    V = f.V
    cpu = lambda x: x.detach().cpu().contiguous()
    conic, y = cpu(f.conic[:V]), cpu(f.opacity_act[:V])
    gen = torch.Generator().manual_seed(FRAME["seed"] + 1)
    base = dict(W=W, H=H, V=V, uv=cpu(f.uv[:V]), conic=conic, coeff16=cpu(f.rgb_render[:V]).reshape(V, 3, 1),
                rays=torch.zeros(H, W, 3), grad_image=torch.randn(H, W, 3, generator=gen),
                bg=torch.full((3,), FRAME["bg"]), sorted_g=cpu(f.sorted_g).int(), ranges=cpu(f.ranges).int())
    sc32 = SimpleNamespace(name="fisheye frame", opacity=y, **base)
    ref = R.render_fp64(base["uv"], y.double(), R.scene_coeff(sc32, 1), conic, base["rays"], base["ranges"],
                        base["sorted_g"], base["bg"], W, H, R.FP32, base["grad_image"])
    ref.grad_image = (base["grad_image"].double() * (~ref.fragile)[:, :, None]).contiguous()
    orc = oracle_run(sc32, 1, torch.float32, ref.grad_image, exact=True)
    # ---- the parameter gradients: float64 chain, carried abs sums, fp32 chain ----
    culled = f.culling_mask.cpu()
    vis = torch.nonzero(~culled).flatten()
    assert vis.shape[0] == V and torch.equal(vis, cpu(f.vis_idx[:V]).long())
    cg = SimpleNamespace(**{k: (None if getattr(g, k) is None else getattr(g, k).detach().cpu()) for k in NAMES})
    scene = SimpleNamespace(g=cg, cam=Camera(W, H, cam.K.cpu()), T=T.cpu(), W=W, H=H, near=d["near_thresh"],
                            far=d["far_thresh"], pad=d["cull_mask_padding"], mh=d["mh_dist"])
    L = F.leaves(cg, torch.float64)
    out = F.per_gaussian_fisheye(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], scene.T,
                                 scene.cam.K, W, H, scene.near, scene.far, scene.pad)
    assert torch.equal(out["culled"], culled)   # (no row of this frame sits on a frustum edge)
    yv = torch.cat([out["rgb_render"][vis], out["opacity_act"][vis], out["uv"][vis], out["conic"][vis]], dim=1)
    slab_of = lambda gr: torch.cat([gr["g_rgb"].reshape(V, 3), gr["g_opacity"], gr["g_uv"], gr["g_conic"]], dim=1).double()
    keys = [k for k in L if L[k] is not None]
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
    param_orc = F.stage(scene, torch.float32, orc_slab, vis)["grad"]
    return SimpleNamespace(ref=ref, orc=orc, param_ref=param_ref, carried=carried, param_orc=param_orc, culled=culled, V=V)


@pytest.mark.parametrize("mode", ["native", "python"])
def test_frame_against_the_fp64_chain(mode):
    """FRAME of tests/test_gpu_render_ref64.py through the fisheye camera: the image by r_measure against render_ref64
    fed the frame's own per-Gaussian outputs (envelope: the fp32 render oracle fed the same), R_MAX = 8; the parameter
    gradients by the noise rule against the float64 chain -- |got - ref| / (abs sums carried through the stage) may
    exceed the fp32 chain's value of the same measure by NOISE_MARGIN = 2e-5 and no more"""
    assert mode == "python" or fused.native() is not None, "native frame module not built"
    fr = frame_reference()
    ref = fr.ref
    ok = ~ref.fragile
    g, cam, T, bg = frame_inputs(grad=True)
    prev = fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT
    fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT = mode == "native", False, False
    try:
        _hip.set_backward_mode("exact")
        image, mask, uv = run_frame(g, cam, T, bg, camera_model="fisheye")
        image.backward(ref.grad_image.float().to(DEV))
        torch.cuda.synchronize()
    finally:
        _hip.set_backward_mode("compat")
        fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT = prev
    assert torch.equal(mask.cpu(), fr.culled)
    n = int(ok.sum())
    img = image.detach().cpu().double()
    vals = {"fragile": float(ref.fragile.float().mean()), "V": fr.V,
            "r_image": r_measure(img[ok].reshape(n, -1), ref.image[ok].reshape(n, -1),
                                 (fr.orc["image"].double() - ref.image)[ok].reshape(n, -1))}
    for k in fr.param_ref:
        got = getattr(g, k).grad.cpu()
        assert not got[fr.culled].any(), k
        vals[f"oracle_{k}"] = noise_measure(fr.param_orc[k], fr.param_ref[k], fr.carried[k])
        vals[f"kernel_{k}"] = noise_measure(got, fr.param_ref[k], fr.carried[k])
    report(f"fisheye_frame[{mode}]", **vals)
    print(f"fisheye_frame[{mode}]", {k: (round(v, 9) if isinstance(v, float) else v) for k, v in vals.items()})
    assert vals["fragile"] <= 0.05
    assert vals["r_image"] <= R_MAX, vals
    for k in fr.param_ref:
        assert vals[f"kernel_{k}"] <= vals[f"oracle_{k}"] + NOISE_MARGIN, (k, vals)
        assert getattr(g, k).grad.abs().max() > 0, k


# ---- 6. training ------------------------------------------------------------------------------------------------------
def test_training_smoke():
    g, cam, T, bg = small_frame()
    with torch.no_grad():
        target = run_frame(g, cam, T, bg, camera_model="fisheye")[0].clone()
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
        loss = (run_frame(gp, cam, T, bg, camera_model="fisheye")[0] - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        final = float((run_frame(gp, cam, T, bg, camera_model="fisheye")[0] - target).abs().mean())
    check("fisheye_training_smoke", dict(initial=losses[0], final=final))
    for k, v in params.items():
        assert bool(torch.isfinite(v).all()), k
    assert final < losses[0]


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_frame_alone():
    g, cam, T, bg = small_frame()
    before = run_frame(g, cam, T, bg)[0].clone()
    before_f = run_frame(g, cam, T, bg, camera_model="fisheye")[0].clone()
    launches = fused.counters()["frames"]
    feat = torch.rand(g.xyz.shape[0], 3, device=DEV)
    refused = [dict(adam_plan=object()), dict(tile_rows=(0, 2)), dict(return_aux=True), dict(grad_sync=lambda t: t),
               dict(slab_sync=lambda t: None), dict(frame_hook=lambda d: None)]
    for kw in refused:
        for fn in (fused.rasterize, fused.rasterize_rgbd, fused.rasterize_distortion, fused.rasterize_contributions):
            with pytest.raises(RuntimeError, match="fisheye|rasterize_rgbd|rasterize_distortion|rasterize_contributions"):
                run_frame(g, cam, T, bg, fn=fn, camera_model="fisheye", **kw)
        with pytest.raises(RuntimeError, match="rasterize_features"):
            fused.rasterize_features(g, feat, T, cam, use_sh_precompute=True, background_rgb=bg, camera_model="fisheye",
                                     **DEFAULTS, **kw)
    with pytest.raises(RuntimeError, match="per-pixel SH"):
        fused.rasterize(g, T, cam, use_sh_precompute=False, background_rgb=bg, camera_model="fisheye", **DEFAULTS)
    g64 = Gaussians(*[None if x is None else x.detach().double() for x in (g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, g.sh)])
    with pytest.raises(RuntimeError, match="float32 tensors on the GPU"):
        fused.rasterize(g64, T.double(), Camera(64, 48, cam.K.double()), use_sh_precompute=True,
                        background_rgb=bg.double(), camera_model="fisheye", **DEFAULTS)
    cpu = Gaussians(*[None if x is None else x.detach().cpu() for x in (g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, g.sh)])
    with pytest.raises(RuntimeError, match="float32 tensors on the GPU"):
        fused.rasterize(cpu, T.cpu(), Camera(64, 48, cam.K.cpu()), use_sh_precompute=True, background_rgb=bg.cpu(),
                        camera_model="fisheye", **DEFAULTS)
    with pytest.raises(RuntimeError, match="tile_rows"):
        fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, 64, 48, 0.3, 500.0, 100,
                                 3.0, (0, 2), 0, camera_model="fisheye")
    with pytest.raises(RuntimeError, match="'pinhole' / 'fisheye'"):
        run_frame(g, cam, T, bg, camera_model="equisolid")
    nat = fused.native()
    if nat is not None:   # the native entry refuses on its own too
        with pytest.raises(RuntimeError, match="raster_mode"):
            nat.rasterize(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, 64, 48, 0.3, 500.0, 100.0, 3.0,
                          bg, 0, -1, 4)
        with pytest.raises(RuntimeError, match="fisheye frames are whole frames"):
            nat.rasterize(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, 64, 48, 0.3, 500.0, 100.0, 3.0,
                          bg, 0, 2, FISH)
    assert fused.counters()["frames"] == launches   # nothing was enqueued by the Python orchestration
    with torch.no_grad():
        assert torch.equal(run_frame(g, cam, T, bg)[0], before)
        assert torch.equal(run_frame(g, cam, T, bg, camera_model="fisheye")[0], before_f)
