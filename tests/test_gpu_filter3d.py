"""fused.rasterize(filter3d=) / the _filtered entries and gs_filter3d_rate (ABI 20): the rate kernel, the per-Gaussian
kernels' F3D instantiations at the stage level, the pose, what the filter is for, the frame through both orchestrations,
a short training run and the refusals.

Stage measures: ref64.r_measure with env = |the fp32 evaluation of tests/filter3d_ref.py's restatement - its float64
evaluation|, bound R_MAX = 8 (tests/test_gpu_general_cameras.py).  The values are compared on the rows the kernel itself
kept.  As in tests/test_gpu_antialias.py the fp32 evaluation takes the 2D factor comp, which cancels, on the conic the
kernels computed (filter3d_ref's conic_bits); the conic itself is held to the float64 chain.  Under antialiased the rows whose `det_0 > 0` decision differs between the two precisions are left out (7e; capped
at 0.5 % in tests/test_filter3d_ref.py); the rate leaves out rows within 1e-3 px of a padded edge or 1e-6 of near.

The scenes' filter is tests/filter3d_ref.py's phi_of with the eight tiny rows overridden: the four of log-scale -20 get
phi = 1, so that rho3 = (4e-18)^3 underflows in fp32 and comp3 == 0 whatever the denormal mode; the four of log-scale -50
get exactly 0 (1e-8 .. 1 times their s^2 = 4e-44 is a denormal or 0 by the draw).  The `phi = 0 rows carry the unfiltered
call's bits` property is checked on the phi == 0 rows whose fp32 s^2 is not zero (s^2 / s^2 is 0 / 0 otherwise; no row of
these scenes is one, log-scale -50 squares to a denormal, which the kernels keep).

Pose: the measure and bound of tests/test_gpu_pose_grad.py with the per-Gaussian terms taken by autograd (one pose per
Gaussian).  Frame: tests/test_gpu_render_ref64.py's image measure and noise rule, the fp32 restatement's chain in the
place of the oracle's."""
import functools
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.splat_py.structs import Camera, Gaussians
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

from . import filter3d_ref as F
from . import render_ref64 as R
from .fisheye_ref import leaves
from .helpers import report
from .pose_terms import pose_r
from .ref64 import LEAVES, SH_0, general_camera_scene, look_at_pose, r_measure, random_slab, to_device
from .test_gpu_render_ref64 import FRAME, NOISE_MARGIN, noise_measure
from .test_render_ref64 import oracle_run

pytestmark = pytest.mark.gpu
DEV = "cuda"
R_MAX = 8.0
NAMES = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
KINDS = [k for k, _ in F.SCENES]
MODE_BITS = {"filter": 0, "filter+aa": 1, "filter+aa+fisheye": 3, "filter+fisheye": 2}
MODE_KW = {"filter": {}, "filter+aa": dict(antialiased=True),
           "filter+aa+fisheye": dict(antialiased=True, camera_model="fisheye"),
           "filter+fisheye": dict(camera_model="fisheye")}


def p(t):
    return None if t is None else t.data_ptr()


def check(tag, rs):
    report(tag, **rs)
    print(tag, {k: round(v, 3) for k, v in rs.items()})
    for k, v in rs.items():
        assert v <= R_MAX, (tag, k, v)


# ---- 1. the rate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["pinhole", "fisheye"])
@pytest.mark.parametrize("C", F.CAMERA_COUNTS)
def test_rate(C, model):
    sc, cams = F.scene("landscape"), F.camera_set("landscape", C)
    fish = model == "fisheye"
    r64, seen, fragile = F.rate_of(sc.g.xyz, cams.Ts, cams.Ks, cams.sizes, fisheye=fish, detail=True)
    r32 = F.rate_of(sc.g.xyz, cams.Ts, cams.Ks, cams.sizes, dtype=torch.float32, fisheye=fish)
    xyz, Ts, Ks, sizes = (x.to(DEV) for x in (sc.g.xyz, cams.Ts, cams.Ks, cams.sizes))
    got = fused.filter3d_rate(xyz, Ts, Ks, sizes, camera_model=model)
    ok = ~fragile
    assert torch.equal(got.cpu()[ok] > 0, r64[ok] > 0)
    r = r_measure(got.cpu()[ok, None], r64[ok, None], (r32.double() - r64)[ok, None])
    tag = f"filter3d_rate[C {C} {model}]"
    report(tag, r=r, left_out=int(fragile.sum()), never_seen=int((r64 == 0).sum()))
    print(f"{tag}: r = {r:.3g}, {int(fragile.sum())} rows left out, {int((r64 == 0).sum())} never seen")
    assert r <= R_MAX, r
    # two calls over halves of the cameras = one call; a tuple for sizes = the tensor
    if C > 1:
        h = C // 2
        part = fused.filter3d_rate(xyz, Ts[:h], Ks[:h], sizes[:h], camera_model=model)
        part = fused.filter3d_rate(xyz, Ts[h:], Ks[h:], sizes[h:], camera_model=model, out=part)
        assert torch.equal(part, got)
    else:
        assert torch.equal(fused.filter3d_rate(xyz, Ts, Ks, (sc.W, sc.H), camera_model=model), got)
    # rows no camera sees keep their input; the others never fall below it
    start = torch.rand(xyz.shape[0], generator=torch.Generator().manual_seed(3)).to(DEV) * 50.0
    out = fused.filter3d_rate(xyz, Ts, Ks, sizes, camera_model=model, out=start.clone())
    never = (~seen.any(dim=0) & ok).to(DEV)
    assert torch.equal(out[never], start[never]) and torch.equal(out, torch.maximum(start, got))


def test_rate_single_row_and_refusals():
    sc, cams = F.scene("landscape"), F.camera_set("landscape", 5)
    Ts, Ks, sizes = (x.to(DEV) for x in (cams.Ts, cams.Ks, cams.sizes))
    vis = int(torch.nonzero(F.rate_of(sc.g.xyz, cams.Ts, cams.Ks, cams.sizes) > 0)[0])
    one = sc.g.xyz[vis:vis + 1].to(DEV)
    got = fused.filter3d_rate(one, Ts, Ks, sizes)
    want = F.rate_of(one, cams.Ts, cams.Ks, cams.sizes)
    assert got.shape == (1,) and abs(float(got) - float(want)) <= 1e-5 * float(want)
    assert fused.filter3d_rate(one[:0], Ts, Ks, sizes).shape == (0,)
    assert not fused.filter3d_rate(one, Ts[:0], Ks[:0], sizes[:0]).any()
    lib = _hip.lib()
    xyz = sc.g.xyz.to(DEV)
    rate = torch.full((xyz.shape[0],), 7.0, device=DEV)
    base = lambda **kw: [kw.get("xyz", p(xyz)), p(Ts), p(Ks), kw.get("sizes", p(sizes)), 5, xyz.shape[0], 0.2, 0.15,
                         kw.get("mode", 0), p(rate), _hip.current_stream()]
    for kw, word in ((dict(mode=1), b"raster_mode"), (dict(mode=3), b"raster_mode"), (dict(mode=4), b"raster_mode"),
                     (dict(xyz=None), b"NULL"), (dict(sizes=None), b"NULL")):
        assert lib.gs_filter3d_rate(*base(**kw)) == _hip.GS_EINVAL and word in lib.gs_last_error(), kw
        torch.cuda.synchronize()
        assert bool((rate == 7.0).all()), kw
    with pytest.raises(RuntimeError, match="camera_model"):
        fused.filter3d_rate(xyz, Ts, Ks, sizes, camera_model="orthographic")
    with pytest.raises(RuntimeError, match="Ks must be"):
        fused.filter3d_rate(xyz, Ts, Ks[:3], sizes)


# ---- stage scenes -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_case(kind, mode):
    """the scene, its filter (four rows overridden, see the module docstring), the kernels' forward, the float64 and the
    fp32 restatement (the latter's 2D factor on the kernels' conic), the rows both precisions decide alike on"""
    sc = F.scene(kind)
    phi = sc.phi.clone()
    phi[sc.tiny[:4]] = 1.0
    phi[sc.tiny[4:]] = 0.0
    g, cam, T = to_device(sc, DEV)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, sc.near,
                                 sc.far, sc.pad, sc.mh, None, 0, filter3d=phi.to(DEV), **MODE_KW[mode])
    torch.cuda.synchronize()
    vis = f.vis_idx[:f.V].cpu().long()
    bits = (vis, f.conic[:f.V].cpu())
    ref, env = F.stage(sc, phi, torch.float64, mode), F.stage(sc, phi, torch.float32, mode, conic_bits=bits)
    s2_32 = torch.exp(sc.g.scale) ** 2
    zero_rows = (phi == 0) & (s2_32.min(dim=1).values > 0)
    flips = (ref["det_0"] > 0) != (env["det_0"] > 0) if MODE_KW[mode].get("antialiased") else torch.zeros_like(zero_rows)
    assert int(zero_rows.sum()) > 50 and int(flips[vis].sum()) <= 0.005 * vis.numel()
    return SimpleNamespace(sc=sc, phi=phi, ref=ref, env=env, zero_rows=zero_rows, ok_g=~flips, comp0_g=sc.tiny[:4],
                           vis=vis, bits=bits, f=f, dev=(g, cam, T))


def raw_forward(sc, g, cam, T, mode_bits, phi, cut, entry="gs_preprocess_forward_filtered"):
    """a per-Gaussian forward entry through the typed loader on buffers of its own; phi None = filter3d NULL
    -> (status, outputs by visible index on the CPU, the visible Gaussians' indices)"""
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
    if entry.endswith("_filtered"):
        args.append(p(phi))
    status = getattr(lib, entry)(*args, mode_bits, _hip.current_stream())
    torch.cuda.synchronize()
    if status != 0:
        return status, None, None
    V = int(o.count)
    c = lambda x: x[:V].cpu()
    got = dict(uv=c(o.uv), xyz_cam=c(o.xc), conic=c(o.conic), opacity_act=c(o.opa), rgb_render=c(o.rgb), packed=c(o.packed),
               vis_idx=c(o.vis), culling_mask=o.mask.cpu().bool(), rank=o.rank.cpu())
    if cut:
        got["bin_rec"] = c(o.bin_rec)
    return status, got, got["vis_idx"].long()


# ---- 2. forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(F.MODES))
@pytest.mark.parametrize("kind", KINDS)
def test_forward(kind, mode):
    case = stage_case(kind, mode)
    sc, bits = case.sc, MODE_BITS[mode]
    g, cam, T = to_device(sc, DEV)
    phi = case.phi.to(DEV)
    s, got, vis = raw_forward(sc, g, cam, T, bits, phi, False)
    assert torch.equal(vis, case.vis) and torch.equal(got["conic"], case.bits[1])   # the frame's stage: the same bits
    s_cut, got_cut, _ = raw_forward(sc, g, cam, T, bits, phi, True)
    s_plain, plain, _ = raw_forward(sc, g, cam, T, bits, None, False, "gs_preprocess_forward_mode")
    s_null, null, _ = raw_forward(sc, g, cam, T, bits, None, False)
    assert (s, s_cut, s_plain, s_null) == (0, 0, 0, 0)
    V = vis.numel()
    assert 0 < V < sc.g.xyz.shape[0]
    for k in got:    # the cut form: the same bits, and the binning records hold them
        assert torch.equal(got[k], got_cut[k]), k
    assert torch.equal(got_cut["bin_rec"][:, 0:2], got["uv"]) and torch.equal(got_cut["bin_rec"][:, 2:5], got["conic"])
    for k in plain:  # filter3d == NULL through the new entry = the _mode entry
        assert torch.equal(null[k], plain[k]), k
    for k in ("uv", "xyz_cam", "opacity_act", "rgb_render", "vis_idx", "culling_mask", "rank"):
        assert torch.equal(got[k], plain[k]), k
    assert torch.equal(got["packed"][:, [0, 1, 9, 10, 11]], plain["packed"][:, [0, 1, 9, 10, 11]])
    zero_v = case.zero_rows[vis]
    assert int(zero_v.sum()) > 30
    for k in ("conic", "packed"):
        assert torch.equal(got[k][zero_v], plain[k][zero_v]), k
    assert not torch.equal(got["conic"][~zero_v], plain["conic"][~zero_v])
    # against the float64 chain
    ok = case.ok_g[vis]
    ref, env = case.ref, case.env
    rs = {"conic": r_measure(got["conic"][ok], ref["conic"][vis][ok], (env["conic"].double() - ref["conic"])[vis][ok]),
          "abc": r_measure(got["packed"][:, 4:7][ok], ref["packed_abc"][vis][ok],
                           (env["packed_abc"].double() - ref["packed_abc"])[vis][ok]),
          "opacity": r_measure(got["packed"][:, 3:4][ok], ref["opa"][vis][ok], (env["opa"].double() - ref["opa"])[vis][ok])}
    check(f"filter3d_forward[{kind} {mode}]", rs)
    assert torch.equal(got["packed"][:, 5], got["conic"][:, 1] * 0.5)
    # comp3 == 0 rows never contribute
    comp0_v = torch.isin(vis, case.comp0_g)
    assert int(comp0_v.sum()) == 4
    assert bool((got["packed"][comp0_v, 2] == -1).all()) and not got["packed"][comp0_v, 3].any()
    if not MODE_KW[mode].get("antialiased"):   # (under antialiased the 2D factor of the wider splat is the larger one)
        assert bool((got["packed"][:, 3] <= plain["packed"][:, 3]).all())


# ---- 3. backward --------------------------------------------------------------------------------------------------------
def stage_forward(case, mode, filtered=True):
    sc = case.sc
    g, cam, T = to_device(sc, DEV)
    phi = case.phi.to(DEV) if filtered else None
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, sc.near,
                                 sc.far, sc.pad, sc.mh, None, 0, filter3d=phi, **MODE_KW[mode])
    torch.cuda.synchronize()
    return f, (g, cam, T), phi


def backward_r(case, got, ref_g, env_g, vis, i0=0, i1=None):
    N = case.sc.g.xyz.shape[0]
    i1 = N if i1 is None else i1
    ok = case.ok_g.clone()[i0:i1]
    culled = torch.ones(N, dtype=torch.bool)
    culled[vis] = False
    culled = culled[i0:i1]
    out = {}
    for k in got:
        if got[k] is None:
            continue
        assert not got[k][culled].any(), k
        assert bool(torch.isfinite(got[k]).all()), k
        r, e = ref_g[k][i0:i1], env_g[k][i0:i1].double()
        out[k] = r_measure(got[k][ok], r[ok], e[ok] - r[ok])
    return out


@pytest.mark.parametrize("mode", list(F.MODES))
@pytest.mark.parametrize("kind", KINDS)
def test_backward(kind, mode):
    case = stage_case(kind, mode)
    sc, kw = case.sc, MODE_KW[mode]
    f, (g, cam, T), phi = stage_forward(case, mode)
    V = f.V
    vis = f.vis_idx[:V].cpu().long()
    slab = random_slab(V, 5)
    ref_g = F.stage(sc, case.phi, torch.float64, mode, slab=slab, rows=vis)["grad"]
    env_g = F.stage(sc, case.phi, torch.float32, mode, slab=slab, rows=vis, conic_bits=case.bits)["grad"]
    slab_d = slab.to(DEV).contiguous()
    cpu = lambda out: {k: (None if x is None else x.cpu()) for k, x in zip(NAMES, out)}
    run = lambda s, filt=phi, fw=f, **more: cpu(fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, fw, s,
                                                                          filter3d=filt, **kw, **more))
    whole = run(slab_d)
    tag = f"filter3d_backward[{kind} {mode}]"
    check(tag + " whole set", backward_r(case, whole, ref_g, env_g, vis))
    i0, i1 = 256, 1792
    v_base = int((vis < i0).sum())
    part = run(slab_d[v_base:].contiguous(), v_base=v_base, i0=i0, i1=i1)
    check(tag + " owner slice", backward_r(case, part, ref_g, env_g, vis, i0, i1))
    for k in part:
        if part[k] is not None:
            assert torch.equal(part[k], whole[k][i0:i1]), k
    # comp3 == 0 rows: opacity gradient 0
    assert not whole["opacity"][case.comp0_g].any()
    # the opacity column alone reaches the scale gradient; without a filter (and without the 2D factor) it cannot
    only3 = torch.zeros_like(slab_d)
    only3[:, 3] = slab_d[:, 3]
    with_filter = run(only3)
    assert bool(with_filter["scale"].any())
    if not kw.get("antialiased"):
        f0, _, _ = stage_forward(case, mode, filtered=False)
        assert not run(only3, None, f0)["scale"].any()
    # phi == 0 rows: the bits of the backward without a filter
    f0, _, _ = stage_forward(case, mode, filtered=False)
    assert torch.equal(f0.vis_idx[:V].cpu().long(), vis)
    plain = run(slab_d, None, f0)
    zero = case.zero_rows
    for k in whole:
        if whole[k] is not None:
            assert torch.equal(whole[k][zero], plain[k][zero]), k
    assert not torch.equal(whole["scale"][~zero], plain["scale"][~zero])


def test_wide_fold_on_both_sides_of_its_threshold():
    """With a filter the antialiased fold forms its conic terms beyond det_d > 1e18 as (c0 - rho c) / det_d (pg_math.h
    aa_fold_row<WIDE>: det_d det_d leaves fp32's range from 1.8e19).  Filters chosen per row so that the kernels' det_d
    (packed column 7) spreads over 1e17 .. 3e19: the backward, whole and through the pose kernel, is finite on every row
    and within the stage bound of the float64 chain, with hundreds of rows on either side of the threshold and beyond
    the plain form's overflow."""
    mode = "filter+aa"
    sc = F.scene("odd")
    g, cam, T = to_device(sc, DEV)
    gen = torch.Generator().manual_seed(41)
    z = (sc.g.xyz @ sc.T[:3, :3].T + sc.T[:3, 3])[:, 2].clamp(min=sc.near)
    target = 10.0 ** (8.5 + 1.25 * torch.rand(z.shape[0], generator=gen))          # conic ~ phi (f / z)^2
    phi = (target * (z / float(sc.cam.K[0, 0])) ** 2).float().contiguous()
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, sc.near,
                                 sc.far, sc.pad, sc.mh, None, 0, filter3d=phi.to(DEV), **MODE_KW[mode])
    V = f.V
    vis = f.vis_idx[:V].cpu().long()
    det_d = f.packed[:V, 7].cpu()
    assert bool(torch.isfinite(det_d).all())
    n_below, n_above, n_past = int((det_d < 1e18).sum()), int((det_d > 1e18).sum()), int((det_d > 2e19).sum())
    assert min(n_below, n_above) > 300 and n_past > 100, (n_below, n_above, n_past)
    bits = (vis, f.conic[:V].cpu())
    slab = random_slab(V, 43)
    ref_g = F.stage(sc, phi, torch.float64, mode, slab=slab, rows=vis)["grad"]
    env_g = F.stage(sc, phi, torch.float32, mode, slab=slab, rows=vis, conic_bits=bits)["grad"]
    case = SimpleNamespace(sc=sc, ok_g=torch.ones(z.shape[0], dtype=torch.bool))
    got = fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab.to(DEV).contiguous(),
                                    filter3d=phi.to(DEV), **MODE_KW[mode])
    got = {k: (None if x is None else x.cpu()) for k, x in zip(NAMES, got)}
    # (the fp32 restatement's own autograd overflows beyond 1.8e19 -- its det_d^2 -- and is no envelope there)
    finite = torch.ones(z.shape[0], dtype=torch.bool)
    for k, e in env_g.items():
        finite &= torch.isfinite(e.reshape(e.shape[0], -1)).all(dim=1)
    case.ok_g = finite
    assert int((det_d[finite[vis]] > 1e18).sum()) > 300
    check(f"filter3d_wide_fold[{n_below} below, {n_above} above, {n_past} past 2e19]", backward_r(case, got, ref_g, env_g, vis))
    pose = fused.pose_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab.to(DEV).contiguous(), filter3d=phi.to(DEV),
                               **MODE_KW[mode])
    assert bool(torch.isfinite(pose).all()) and bool(pose[:3].any())


# ---- 4. pose ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(F.MODES))
@pytest.mark.parametrize("kind", KINDS)
def test_pose(kind, mode):
    """gs_pose_backward_filtered against float64 autograd through the filtered stage: r = |got - sum t64| / (E + 2^-22 B)
    over the per-Gaussian terms t (tests/test_gpu_pose_grad.py), t64 / t32 = the gradient of one pose per Gaussian in
    either precision.  The kernel without the filter on the same slab misses the bound by orders of magnitude."""
    case = stage_case(kind, mode)
    sc, kw = case.sc, MODE_KW[mode]
    f, (g, cam, T), phi = stage_forward(case, mode)
    V = f.V
    vis = f.vis_idx[:V].cpu().long()
    slab = random_slab(V, 17)
    slab[~case.ok_g[vis]] = 0   # rows the two precisions decide differently on carry nothing
    t64 = F.stage(sc, case.phi, torch.float64, mode, slab=slab, rows=vis, pose_terms=True)["pose_terms"]
    t32 = F.stage(sc, case.phi, torch.float32, mode, slab=slab, rows=vis, pose_terms=True,
                  conic_bits=case.bits)["pose_terms"].double()
    ref, B, E = t64.sum(0), t64.abs().sum(0), (t32 - t64).abs().sum(0)
    run = lambda filt: fused.pose_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab.to(DEV).contiguous(),
                                           filter3d=filt, **kw)
    got, again = run(phi), run(phi)
    assert torch.equal(got, again) and not got[3].any() and bool(torch.isfinite(got).all())
    r, r_plain = pose_r(got, ref, B, E), pose_r(run(None), ref, B, E)
    report(f"filter3d_pose[{kind} {mode}]", r=r, r_of_the_kernel_without_the_filter=r_plain)
    print(f"filter3d_pose[{kind} {mode}]: r = {r:.3g} (the kernel without the filter on the same slab: {r_plain:.3g})")
    assert r <= R_MAX, r
    assert r_plain > 100 * R_MAX, r_plain


# ---- 5. what it is for --------------------------------------------------------------------------------------------------
def test_filtered_splats_are_no_smaller_than_the_sampling_interval():
    sc = general_camera_scene(171, 3000, deg=0, kind="landscape", stress=False, fy_over_fx=1.0)
    gen = torch.Generator().manual_seed(172)
    target = sc.g.xyz.double().mean(dim=0)
    Ts = [sc.T.double()]
    for _ in range(4):
        A, centre = look_at_pose(gen, target, 4.0 + 12.0 * float(torch.rand(1, generator=gen, dtype=torch.float64)))
        T = torch.eye(4, dtype=torch.float64)
        T[:3, :3], T[:3, 3] = A, -A @ centre
        Ts.append(T)
    g, cam, _ = to_device(sc, DEV)
    Ts = torch.stack(Ts).float().to(DEV)
    Ks = cam.K[None].repeat(5, 1, 1).contiguous()
    rate = fused.filter3d_rate(g.xyz, Ts, Ks, (sc.W, sc.H))
    phi = fused.filter3d_from_rate(rate, 0.2)
    assert bool((rate > 0).any()) and bool(torch.isfinite(phi).all())
    s2 = torch.exp(g.scale.double()) ** 2
    checked = 0
    for k in range(5):
        f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, Ts[k], cam.K, sc.W, sc.H, sc.near,
                                     sc.far, sc.pad, sc.mh, None, 0, filter3d=phi)
        V = f.V
        vis = f.vis_idx[:V].long()
        own = fused.filter3d_rate(g.xyz, Ts[k:k + 1], Ks[k:k + 1], (sc.W, sc.H))
        sel = ((own == rate) & (rate > 0))[vis]
        c = f.conic[:V].double()[sel]
        half, b = 0.5 * (c[:, 0] + c[:, 2]), 0.5 * c[:, 1]
        lmin = half - torch.sqrt((0.5 * (c[:, 0] - c[:, 2])) ** 2 + b * b)
        checked += int(sel.sum())
        assert bool((lmin >= 0.2 * (1 - 1e-4)).all()), (k, float(lmin.min()))
        # opa3 sqrt(det Sigma_eff) = y prod s
        lhs = f.packed[:V, 3].double() * torch.sqrt((s2 + phi.double()[:, None]).prod(dim=1))[vis]
        rhs = f.opacity_act[:V, 0].double() * torch.sqrt(s2.prod(dim=1))[vis]
        assert float(((lhs - rhs).abs() / rhs).max()) < 1e-5
    assert checked > 1000


# ---- 6. frame -----------------------------------------------------------------------------------------------------------
PARAMS = ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")
FRAME_KW = dict(antialiased=True)


def frame_inputs(grad=False):
    c = FRAME
    g, cam, T = make_scene(c["N"], c["W"], c["H"], 1, seed=c["seed"], device=DEV)
    g.opacity.add_(c["shift"])
    rate = fused.filter3d_rate(g.xyz, T[None].contiguous(), cam.K[None].contiguous(), (c["W"], c["H"]))
    phi = fused.filter3d_from_rate(rate, 0.2)
    if grad:
        for k in PARAMS:
            getattr(g, k).requires_grad_(True)
    return g, cam, T, torch.full((3,), c["bg"], device=DEV), phi


def opa_of(conic, y, log_scale, phi, dtype):
    """the record's opacity of the antialiased filtered frame from the frame's own conic and sigmoid, in dtype"""
    comp, _ = F.aa_comp(conic.to(dtype))
    return y.to(dtype).reshape(-1, 1) * F.comp3_of(log_scale.to(dtype), phi.to(dtype))[:, None] * comp[:, None]


@functools.lru_cache(maxsize=None)
def frame_reference():
    g, cam, T, bg, phi = frame_inputs()
    W, H = FRAME["W"], FRAME["H"]
    d = DEFAULTS
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, d["near_thresh"],
                                 d["far_thresh"], d["cull_mask_padding"], d["mh_dist"], None, 0, filter3d=phi, **FRAME_KW)
    torch.cuda.synchronize()
    V = f.V
    cpu = lambda x: x.detach().cpu().contiguous()
    vis = cpu(f.vis_idx[:V]).long()
    conic, y = cpu(f.conic[:V]), cpu(f.opacity_act[:V])
    gen = torch.Generator().manual_seed(FRAME["seed"] + 1)
    base = dict(W=W, H=H, V=V, uv=cpu(f.uv[:V]), conic=conic, coeff16=cpu(f.rgb_render[:V]).reshape(V, 3, 1),
                rays=torch.zeros(H, W, 3), grad_image=torch.randn(H, W, 3, generator=gen),
                bg=torch.full((3,), FRAME["bg"]), sorted_g=cpu(f.sorted_g).int(), ranges=cpu(f.ranges).int())
    scale_v, phi_v = cpu(g.scale)[vis], cpu(phi)[vis]
    opa64 = opa_of(conic, y, scale_v, phi_v, torch.float64)
    opa32 = opa_of(conic, y, scale_v, phi_v, torch.float32)
    sc32 = SimpleNamespace(name="filtered frame", opacity=opa32, **base)
    ref = R.render_fp64(base["uv"], opa64, R.scene_coeff(sc32, 1), conic, base["rays"], base["ranges"], base["sorted_g"],
                        base["bg"], W, H, R.FP32, base["grad_image"])
    ref.grad_image = (base["grad_image"].double() * (~ref.fragile)[:, :, None]).contiguous()
    orc = oracle_run(sc32, 1, torch.float32, ref.grad_image, exact=True)
    # the parameter gradients: float64 chain, carried abs sums, the fp32 restatement's chain
    cg = Gaussians(*[None if getattr(g, k) is None else getattr(g, k).detach().cpu() for k in PARAMS])
    scene = SimpleNamespace(g=cg, cam=Camera(W, H, cam.K.cpu()), T=T.cpu(), W=W, H=H, near=d["near_thresh"],
                            far=d["far_thresh"], pad=d["cull_mask_padding"], mh=d["mh_dist"])
    phi_c = cpu(phi)
    slab_of = lambda gr: torch.cat([gr["g_rgb"].reshape(V, 3), gr["g_opacity"], gr["g_uv"], gr["g_conic"]], dim=1).double()
    param_ref = F.stage(scene, phi_c, torch.float64, "filter+aa", slab=slab_of(ref.grad_walk), rows=vis)["grad"]
    a_slab = slab_of(ref.abs_walk)
    L = leaves(cg, torch.float64)
    out = F.filtered_stage(L["xyz"], L["quaternion"], L["scale"], L["opacity"], L["rgb"], L["sh"], phi_c.double(), scene.T,
                           scene.cam.K, W, H, scene.near, scene.far, scene.pad, torch.float64, True, False)
    yv = torch.cat([out["rgb_render"][vis], out["opa"][vis], out["uv"][vis], out["conic"][vis]], dim=1)
    keys = [k for k in LEAVES if L[k] is not None]
    carried = {k: torch.zeros_like(L[k]) for k in keys}
    for j in range(9):
        go = torch.zeros_like(yv)
        go[:, j] = a_slab[:, j]
        for k, x in zip(keys, torch.autograd.grad(yv, [L[k] for k in keys], grad_outputs=go, retain_graph=True,
                                                  allow_unused=True)):
            if x is not None:
                carried[k] += x.detach().abs()
    orc_slab = torch.cat([orc["g_rgb"].reshape(V, 3), orc["g_opacity"], orc["g_uv"], orc["g_conic"]], dim=1).float()
    param_orc = F.stage(scene, phi_c, torch.float32, "filter+aa", slab=orc_slab, rows=vis, conic_bits=(vis, conic))["grad"]
    culled = torch.ones(cg.xyz.shape[0], dtype=torch.bool)
    culled[vis] = False
    return SimpleNamespace(ref=ref, orc=orc, param_ref=param_ref, carried=carried, param_orc=param_orc, culled=culled, V=V)


def image_r(got, want, orc, ok):
    n = int(ok.sum())
    return r_measure(got.double()[ok].reshape(n, -1), want[ok].reshape(n, -1), (orc.double() - want)[ok].reshape(n, -1))


def run_frame(g, cam, T, bg, fn=None, **kw):
    fn = fused.rasterize if fn is None else fn
    return fn(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS, **kw)


@pytest.mark.parametrize("mode", ["native", "python"])
def test_frame_against_the_fp64_chain(mode):
    assert fused.native() is not None, "the native frame module is part of the build"
    fr = frame_reference()
    ref = fr.ref
    ok = ~ref.fragile
    g, cam, T, bg, phi = frame_inputs(grad=True)
    prev = fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT
    fused.NATIVE, fused.SEGMENTS, fused.DEPTH_CUT = mode == "native", False, False
    try:
        _hip.set_backward_mode("exact")
        image, mask, uv = run_frame(g, cam, T, bg, filter3d=phi, **FRAME_KW)
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
        vals[f"restated_{k}"] = noise_measure(fr.param_orc[k], fr.param_ref[k], fr.carried[k])
        vals[f"kernel_{k}"] = noise_measure(got, fr.param_ref[k], fr.carried[k])
    report(f"filter3d_frame[{mode}]", **vals)
    print(f"filter3d_frame[{mode}]", {k: (round(v, 9) if isinstance(v, float) else v) for k, v in vals.items()})
    assert vals["fragile"] <= 0.05
    assert vals["r_image"] <= R_MAX, vals
    for k in fr.param_ref:
        assert vals[f"kernel_{k}"] <= vals[f"restated_{k}"] + NOISE_MARGIN, (k, vals)
        assert getattr(g, k).grad.abs().max() > 0, k


def test_frame_orchestrations_policies_maps_and_bake_agree():
    fr = frame_reference()
    g, cam, T, bg, phi = frame_inputs()
    images = {}
    assert fused.native() is not None, "the native frame module is part of the build"
    prev = fused.NATIVE, fused.DEPTH_CUT
    try:
        for native in (True, False):
            for cut in (False, True):
                fused.NATIVE, fused.DEPTH_CUT = native, cut
                before = fused.counters()["depth_cut_frames"]
                images[(native, cut)] = run_frame(g, cam, T, bg, filter3d=phi, **FRAME_KW)[0]
                assert fused.counters()["depth_cut_frames"] - before == int(cut), (native, cut)
    finally:
        fused.NATIVE, fused.DEPTH_CUT = prev
    first = images[(False, False)]
    for key, img in images.items():
        assert torch.equal(img, first), key
    plain = run_frame(g, cam, T, bg, **FRAME_KW)[0]
    assert torch.equal(run_frame(g, cam, T, bg, filter3d=None, **FRAME_KW)[0], plain) and not torch.equal(plain, first)
    # a filter of zeros is the frame without one; absgrad combines
    assert torch.equal(run_frame(g, cam, T, bg, filter3d=torch.zeros_like(phi), **FRAME_KW)[0], plain)
    assert torch.equal(run_frame(g, cam, T, bg, filter3d=phi, absgrad=True, **FRAME_KW)[0], first)
    # the map entries return rasterize's image
    image_d = run_frame(g, cam, T, bg, fn=fused.rasterize_rgbd, filter3d=phi, **FRAME_KW)[0]
    image_x = run_frame(g, cam, T, bg, fn=fused.rasterize_distortion, filter3d=phi, **FRAME_KW)[0]
    image_c = run_frame(g, cam, T, bg, fn=fused.rasterize_contributions, filter3d=phi, **FRAME_KW)[0]
    feat = torch.rand(g.xyz.shape[0], 3, device=DEV)
    image_f = fused.rasterize_features(g, feat, T, cam, use_sh_precompute=True, background_rgb=bg, filter3d=phi, **FRAME_KW,
                                       **DEFAULTS)[0]
    for img in (image_d, image_x, image_c, image_f):
        assert torch.equal(img, first)
    # the baked Gaussians through the plain frame show the same scene
    ok = ~fr.ref.fragile
    with torch.no_grad():
        baked = fused.bake_filter3d(g, phi)
        image_b = run_frame(baked, cam, T, bg, **FRAME_KW)[0]
    r_first = image_r(first.cpu(), fr.ref.image, fr.orc["image"], ok)
    r_baked = image_r(image_b.cpu(), fr.ref.image, fr.orc["image"], ok)
    mutual = float((image_b - first).abs().max())
    report("filter3d_frame[baked]", r_image=r_first, r_baked=r_baked, mutual_max_abs=mutual)
    print(f"filter3d_frame[baked]: r = {r_baked:.3g} (the filtered frame: {r_first:.3g}), largest mutual difference {mutual:.3g}")
    assert r_first <= R_MAX and r_baked <= R_MAX, (r_first, r_baked)


# ---- 7. training --------------------------------------------------------------------------------------------------------
def test_training_smoke():
    N, W, H = 3000, 64, 48
    g, cam, T = make_scene(N, W, H, 1, seed=11, device=DEV)
    bg = torch.full((3,), 0.5, device=DEV)
    phi = fused.filter3d_from_rate(fused.filter3d_rate(g.xyz, T[None].contiguous(), cam.K[None].contiguous(), (W, H)))
    kw = dict(antialiased=True, filter3d=phi)
    with torch.no_grad():
        target = run_frame(g, cam, T, bg, **kw)[0].clone()
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
        loss = (run_frame(gp, cam, T, bg, **kw)[0] - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        final = float((run_frame(gp, cam, T, bg, **kw)[0] - target).abs().mean())
    report("filter3d_training_smoke", initial=losses[0], final=final)
    print(f"filter3d_training_smoke: loss {losses[0]:.5f} -> {final:.5f}")
    for k, v in params.items():
        assert bool(torch.isfinite(v).all()), k
    assert final < losses[0]


# ---- 8. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_frame_alone():
    g, cam, T = make_scene(3000, 64, 48, 1, seed=11, device=DEV)
    bg = torch.full((3,), 0.5, device=DEV)
    phi = torch.full((3000,), 1e-4, device=DEV)
    before = run_frame(g, cam, T, bg)[0].clone()
    before_f = run_frame(g, cam, T, bg, filter3d=phi)[0].clone()
    assert not torch.equal(before, before_f)
    refused = [dict(adam_plan=object()), dict(tile_rows=(0, 2)), dict(return_aux=True), dict(grad_sync=lambda t: t),
               dict(slab_sync=lambda t: None), dict(frame_hook=lambda d: None)]
    for kw in refused:
        for fn in (fused.rasterize, fused.rasterize_rgbd, fused.rasterize_distortion, fused.rasterize_contributions):
            with pytest.raises(RuntimeError, match="filter3d|rasterize_"):
                run_frame(g, cam, T, bg, fn=fn, filter3d=phi, **kw)
    with pytest.raises(RuntimeError, match="per-pixel SH"):
        fused.rasterize(g, T, cam, use_sh_precompute=False, background_rgb=bg, filter3d=phi, **DEFAULTS)
    bad = [(phi[:-1], "float32 \\[N\\]"), (phi.double(), "float32 \\[N\\]"), (phi.cpu(), "float32 \\[N\\]"),
           (phi[:, None], "float32 \\[N\\]"), (phi.clone().requires_grad_(True), "must not require a gradient")]
    for t, word in bad:
        for fn in (fused.rasterize, fused.rasterize_rgbd):
            with pytest.raises(RuntimeError, match="filter3d.*" + word):
                run_frame(g, cam, T, bg, fn=fn, filter3d=t)
    with pytest.raises(RuntimeError, match="filter3d must have shape"):
        fused.validate(g, T, cam, bg, phi[:-1])
    g64 = Gaussians(*[None if x is None else x.detach().double() for x in (g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, g.sh)])
    with pytest.raises(RuntimeError, match="float32 tensors on the GPU"):
        fused.rasterize(g64, T.double(), Camera(64, 48, cam.K.double()), use_sh_precompute=True,
                        background_rgb=bg.double(), filter3d=phi, **DEFAULTS)
    # the native entry refuses on its own
    nat = fused.native()
    assert nat is not None, "the native frame module is part of the build"
    d = DEFAULTS
    args = (g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, 64, 48, d["near_thresh"], d["far_thresh"],
            d["cull_mask_padding"], d["mh_dist"], bg)
    for t, word in ((phi[:-1], "float32 \\[N\\]"), (phi.double(), "float32 \\[N\\]"), (phi.cpu(), "float32 \\[N\\]"),
                    (phi.clone().requires_grad_(True), "must not require a gradient")):
        with pytest.raises(RuntimeError, match=word):
            nat.rasterize(*args, 0, -1, 0, t)
    with pytest.raises(RuntimeError, match="whole frames"):
        nat.rasterize(*args, 0, 2, 0, phi)
    with pytest.raises(RuntimeError, match="raster_mode"):
        nat.rasterize(*args, 0, -1, 4, phi)
    assert torch.equal(nat.rasterize(*args, 0, -1, 0, phi)[0], before_f)
    with torch.no_grad():
        assert torch.equal(run_frame(g, cam, T, bg)[0], before)
        assert torch.equal(run_frame(g, cam, T, bg, filter3d=phi)[0], before_f)
