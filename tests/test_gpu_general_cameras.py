"""Every entry point of the per-Gaussian stage on general cameras (fx != fy, off-centre principal point, arbitrary
rotation, camera centre ~20 from the origin, the stress rows of tests/ref64.py) against the float64 reference.

Error measure, per element: r = |hip - ref64| / (env + 2^-22 |ref64| + 1e-7 max|ref64 column|), env = |oracle_fp32 -
ref64| (tests/ref64.py: r_measure); asserted max r <= 8.  The cull mask equals the fp32 oracle's bit for bit;
Gaussians whose fp64 decision differs (fewer than 1e-4 of N) are left out of the fp64 comparisons."""
import ctypes

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.sharded import band_of, owner_blocks
from gaussian_splatting_amd.synthetic import make_grad_image
from oracle import gs_oracle

from .cut_ref import cut_reference, sortable
from .helpers import report
from .ref64 import (KINDS, general_camera_scene, oracle_stages, oracle_vjp, r_measure, random_slab, ref64_abs_vjp,
                    ref64_stage, to_device)
from .test_gpu_band_frontend import run_new, run_old
from .test_gpu_depth_cut import cut_views
from .test_gpu_fused import cpu_expected_stages

pytestmark = pytest.mark.gpu
DEV = "cuda"
R_MAX = 8.0
N_SMALL = 6000   # (> 128 per tile on the one-tile frames: the depth-cut binning admits them)
FWD = (("uv", "uv"), ("xyz_cam", "xyz_c"), ("conic", "conic"), ("opacity_act", "opacity"), ("rgb_render", "rgb"))


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Case:
    """one scene with its fp32 oracle stages, ref64 and the Gaussians both decide alike on"""

    def __init__(self, sc, slab_seed=None, lists=False):
        self.sc = sc
        self.st = oracle_stages(sc, torch.float32, lists=lists)
        self.keep = self.st["keep"]
        self.V = self.st["V"]
        self.vis_g = torch.nonzero(self.keep).flatten()
        self.slab = random_slab(self.V, slab_seed) if slab_seed is not None else None
        self.ref = ref64_stage(sc, self.slab, self.vis_g if self.slab is not None else None)
        differ = self.ref["culled"] != self.st["culled"]
        N = sc.g.xyz.shape[0]
        assert int(differ.sum()) < max(1e-4 * N, 1), int(differ.sum())
        self.agree_v = ~differ[self.vis_g]      # visible rows (by visible index) both precisions keep
        st = self.st
        c = st["conic"]
        self.st_abc = torch.stack([c[:, 0] + 0.25, c[:, 1] * 0.5, c[:, 2] + 0.25], dim=1)

    def forward_r(self, got, v_rows=None):
        """max r of every forward tensor; got: dict of CPU tensors by visible index (rows v_rows of the visible set)"""
        v = torch.arange(self.V) if v_rows is None else v_rows.long()
        sel = self.agree_v[v]
        v, gi = v[sel], self.vis_g[v[sel]]
        out = {}
        for k, ko in FWD:
            out[k] = r_measure(got[k][sel], self.ref[k][gi], self.st[ko][v] - self.ref[k][gi])
        pk = got["packed"][sel]
        out["packed_uv"] = r_measure(pk[:, 0:2], self.ref["uv"][gi], self.st["uv"][v] - self.ref["uv"][gi])
        out["packed_abc"] = r_measure(pk[:, 4:7], self.ref["packed_abc"][gi], self.st_abc[v] - self.ref["packed_abc"][gi])
        return out

    def backward_r(self, got, i0=0, i1=None, slab=None, v_rows=None):
        """max r of the six dense gradients of Gaussians [i0, i1) from the render gradients `slab` of the visible rows
        v_rows (default: the case's slab for every visible row)"""
        sc = self.sc
        N = sc.g.xyz.shape[0]
        i1 = N if i1 is None else i1
        if slab is None:
            ref_g, env_src = self.ref["grad"], oracle_vjp(sc, self.st, self.slab)
        else:
            full = torch.zeros(self.V, 9)
            full[v_rows.long()] = slab
            ref_g = ref64_stage(sc, full, self.vis_g)["grad"]
            env_src = oracle_vjp(sc, self.st, full)
        ok = torch.ones(N, dtype=torch.bool)
        ok[self.vis_g[~self.agree_v]] = False
        ok = ok[i0:i1]
        out = {}
        for k in got:
            if got[k] is None:
                continue
            r, e = ref_g[k][i0:i1], env_src[k][i0:i1].double()
            culled = self.st["culled"][i0:i1]
            assert not got[k][culled].any(), k
            out[k] = r_measure(got[k][ok], r[ok], e[ok] - r[ok])
        return out


def check(tag, rs):
    report(tag, **rs)
    for k, v in rs.items():
        assert v <= R_MAX, (tag, k, v)


def single_gpu_forward(sc, depth_cut=False):
    g, cam, T = to_device(sc, DEV)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, sc.near,
                                 sc.far, sc.pad, sc.mh, None, False, depth_cut=depth_cut)
    torch.cuda.synchronize()
    V = f.V
    c = lambda x: x[:V].detach().cpu()
    got = dict(uv=c(f.uv), xyz_cam=c(f.xyz_cam), conic=c(f.conic), opacity_act=c(f.opacity_act),
               rgb_render=c(f.rgb_render), packed=c(f.packed))
    return f, got, (g, cam, T)


def band_rows(H, G):
    nty = (H + 15) // 16
    return [band_of(nty, G, r)[0] for r in range(G)] + [nty]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_forward_of_every_entry_point_against_ref64(kind, deg):
    sc = general_camera_scene(30 + deg, N_SMALL, deg=deg, kind=kind)
    case = Case(sc, lists=True)
    exp = case.st   # the fp32 oracle stages and lists (cpu_expected_stages)
    tag = f"general_camera[{kind} deg {deg}]"
    V = case.V
    # ---- gs_preprocess_forward and its depth-cut form: bit-equal to the CPU restatement, r against ref64 ----------
    single = {}
    ntx, nty = (sc.W + 15) // 16, (sc.H + 15) // 16
    cut_ok = bool(_hip.lib().gs_cut_supported(ntx, 0, nty, N_SMALL))   # the depth cut's LDS-histogram regime
    for cut in (False, True) if cut_ok else (False,):
        f, got, _ = single_gpu_forward(sc, depth_cut=cut)
        assert f.V == V == exp["V"]
        assert torch.equal(f.culling_mask.cpu(), exp["culled"])
        assert torch.equal(f.vis_idx[:V].cpu().long(), case.vis_g)
        assert torch.equal(got["uv"], exp["uv"]) and torch.equal(got["xyz_cam"], exp["xyz_c"])
        assert torch.equal(got["conic"], exp["conic"]) and torch.equal(got["opacity_act"][:, 0], exp["opacity"].reshape(-1))
        assert (got["rgb_render"] - exp["rgb"]).abs().max() <= 2e-6 * max(1.0, float(exp["rgb"].abs().max()))
        if not cut:
            assert torch.equal(f.ranges.cpu(), exp["ranges"]) and torch.equal(f.sorted_g.cpu(), exp["sorted"])
        check(tag + (" gs_preprocess_forward_cut" if cut else " gs_preprocess_forward"), case.forward_r(got))
        if cut:
            for k in got:
                assert torch.equal(got[k], single[k]), k
            # the cut's lists: depth prefixes of the oracle's complete lists, cut where tests/cut_ref.py cuts them
            bstar, totals, bounds, _, ctrl = (x.cpu() for x in cut_views(f))
            ref = cut_reference(exp["ranges"], exp["sorted"], sortable(exp["xyz_c"][:, 2]), bounds)
            assert torch.equal(f.cut.full_ranges.cpu().long(), exp["ranges"].long()) and f.cut.S_full == int(exp["ranges"][-1])
            assert torch.equal(totals.long(), ref.totals) and int(ctrl[0]) == ref.deepest
            assert torch.equal(bstar.long()[ref.totals > 0], ref.bstar[ref.totals > 0])
            assert torch.equal(f.ranges.cpu().long(), ref.kept_ranges)
            assert torch.equal(f.sorted_g.cpu().long(), ref.kept_sorted)
        single = got
    # ---- the band paths: gs_band_project + gs_preprocess_forward_list, gs_band_frontend ---------------------------
    g, cam, T = to_device(sc, DEV)
    N = sc.g.xyz.shape[0]
    for G, ranks in ((2, (0, 1)), (3, (0, 2))):
        rows = band_rows(sc.H, G)
        oblk = owner_blocks(N, G)
        for me in ranks:
            old = run_old(g, cam, T, sc.W, sc.H, G, me, rows, oblk)
            new = run_new(g, cam, T, sc.W, sc.H, G, me, rows, oblk)
            torch.cuda.synchronize()
            L = int(old["plan"][0])
            assert int(old["plan"][1]) == V and int(new["plan"][0]) == L
            assert torch.equal(old["culled"].cpu().bool(), exp["culled"]) and torch.equal(new["culled"].cpu().bool(), exp["culled"])
            send = old["send"][:L].cpu().long()
            assert torch.equal(new["send"][:L].cpu().long(), send)
            for name, out in (("gs_preprocess_forward_list", old), ("gs_band_frontend", new)):
                lst = dict(uv=out["uv_l"][:L].cpu(), xyz_cam=out["xyz_l"][:L].cpu(), conic=out["conic_l"][:L].cpu(),
                           packed=out["packed_l"][:L].cpu())
                # the documented identity: the rows are the single-GPU rows of the same visible Gaussians, bit for bit
                for k in ("uv", "xyz_cam", "conic", "packed"):
                    assert torch.equal(lst[k], single[k][send]), (name, G, me, k)
                # (the list forms keep sigmoid(opacity) by visible index and the colour only inside the packed record)
                lst["opacity_act"], lst["rgb_render"] = single["opacity_act"][send], single["rgb_render"][send]
                rs = case.forward_r(lst, send)
                check(f"{tag} {name} G={G} rank {me}", rs)


@pytest.mark.parametrize("kind,deg", [("landscape", 3), ("portrait", 0), ("odd", 2), ("one_tile_high", 1),
                                      ("one_tile_wide", 3)])
def test_backward_of_every_entry_point_against_ref64(kind, deg):
    sc = general_camera_scene(40 + deg, N_SMALL, deg=deg, kind=kind)
    case = Case(sc, slab_seed=5)
    tag = f"general_camera[{kind} deg {deg}]"
    f, _, (g, cam, T) = single_gpu_forward(sc)
    N, V = sc.g.xyz.shape[0], case.V
    slab = case.slab.to(DEV).contiguous()
    names = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
    # whole set
    out = fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab)
    torch.cuda.synchronize()
    got = {k: (None if x is None else x.cpu()) for k, x in zip(names, out)}
    check(tag + " gs_preprocess_backward", case.backward_r(got))
    # an owner slice: Gaussians [i0, i1), slab rows from v_base
    i0, i1 = 256, min(N, 256 * 7)
    v_base = int(case.keep[:i0].sum())   # the visible index of the slice's first visible Gaussian
    out = fused.preprocess_backward(g.xyz, g.quaternion, g.scale, T, cam.K, f, slab[v_base:].contiguous(), v_base=v_base,
                                    i0=i0, i1=i1)
    torch.cuda.synchronize()
    got = {k: (None if x is None else x.cpu()) for k, x in zip(names, out)}
    check(tag + " gs_preprocess_backward owner slice", case.backward_r(got, i0, i1))
    # gs_preprocess_backward_gathered at G = 2: rows delivered by both senders, summed on the spot
    G = 2
    rows = band_rows(sc.H, G)
    oblk = owner_blocks(N, G)
    n_sh = 1 if sc.g.sh is None else sc.g.sh.shape[2] + 1
    for me in range(G):
        new = run_new(g, cam, T, sc.W, sc.H, G, me, rows, oblk)
        torch.cuda.synchronize()
        plan = new["plan"].tolist()
        recv_counts = plan[4 + G:4 + 2 * G]
        v_lo, v_hi = plan[2], plan[3]
        n_recv = max(sum(recv_counts), 1)
        recv = random_slab(n_recv, seed=11 + me).to(DEV)
        offs = (ctypes.c_int32 * G)(*[sum(recv_counts[:s]) for s in range(G)])
        owner = (ctypes.c_int32 * (G + 1))(*oblk)
        n_own = v_hi - v_lo
        summed = torch.zeros(max(n_own, 1), 9, device=DEV)
        _hip.call("gs_band_gather_sum", p(new["ws"]), N, G, me, owner, p(new["rank"]), v_lo, p(recv), offs, p(summed),
                  _hip.current_stream())
        i0, i1 = min(N, 256 * oblk[me]), min(N, 256 * oblk[me + 1])
        n = i1 - i0
        grads = [torch.full((n, w), 5.0, device=DEV) for w in (3, 4, 3, 1, 3)] + \
                [torch.full((n, 3, n_sh - 1), 5.0, device=DEV) if n_sh > 1 else None]
        sl = lambda t, w: ctypes.c_void_p(t.data_ptr() + 4 * w * i0)
        _hip.call("gs_preprocess_backward_gathered", sl(g.xyz, 3), sl(g.quaternion, 4), sl(g.scale, 3), n_sh, p(T),
                  p(cam.K), p(new["center"]), ctypes.c_void_p(new["rank"].data_ptr() + 4 * i0), p(new["opa"]),
                  p(new["ws"]), N, G, me, owner, p(recv), offs, n, *[p(x) for x in grads], _hip.current_stream())
        torch.cuda.synchronize()
        got = {k: (None if x is None else x.cpu()) for k, x in zip(names, grads)}
        rs = case.backward_r(got, i0, i1, slab=summed[:n_own].cpu(), v_rows=torch.arange(v_lo, v_hi))
        check(f"{tag} gs_preprocess_backward_gathered G=2 rank {me}", rs)
        if sum(recv_counts) > 0:
            assert any(bool((x != 0).any()) for x in grads if x is not None)


@pytest.mark.parametrize("fy_over_fx", [0.8, 1.25])
@pytest.mark.parametrize("G", [2, 3, 8])
def test_band_masks_are_supersets_of_the_exact_windows(G, fy_over_fx):
    """gs_band_project's and gs_band_frontend's band masks contain every band the exact candidate window of a visible
    Gaussian reaches (gs_oracle.band_mask of the fp32 stages), on general cameras with fx / fy at the range's ends;
    the exact windows of the single-GPU stage (gs_halo_plan) equal the oracle's"""
    from gaussian_splatting_amd.sharded import enqueue_hip_plan, plan_record_ints
    sc = general_camera_scene(50 + G, 60_000, 640, 480, deg=0, fy_over_fx=fy_over_fx, stress=False)
    # a fifth of the Gaussians isotropic: the bound is tight for them, so a Jacobian built from the wrong focal length
    # misses bands
    gen = torch.Generator().manual_seed(G)
    iso = torch.rand(sc.g.xyz.shape[0], generator=gen) < 0.2
    sc.g.scale[iso] = sc.g.scale[iso].mean(dim=1, keepdim=True)
    st = oracle_stages(sc, torch.float32)
    V = st["V"]
    nty = (sc.H + 15) // 16
    rows = band_rows(sc.H, G)
    exact = gs_oracle.band_mask(st["uv"], st["conic"], (sc.W + 15) // 16, nty, sc.mh, rows)
    g, cam, T = to_device(sc, DEV)
    N = sc.g.xyz.shape[0]
    oblk = owner_blocks(N, G)
    me = G // 2
    old = run_old(g, cam, T, sc.W, sc.H, G, me, rows, oblk)
    new = run_new(g, cam, T, sc.W, sc.H, G, me, rows, oblk)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, sc.W, sc.H, sc.near,
                                 sc.far, sc.pad, sc.mh, (rows[me], rows[me + 1]), 0,
                                 plan=lambda fr: enqueue_hip_plan(fr, G, me), plan_ints=plan_record_ints(G))
    torch.cuda.synchronize()
    assert f.V == V
    assert torch.equal(f.halo_mask[:V].cpu(), exact), "the exact windows differ from the oracle's"
    bound_old = old["mask"][:V].cpu()
    nb = (N + 255) // 256
    gm = new["ws"][2 * (G + 1) * (nb + 1):].view(torch.int16)[:N].to(torch.int32) & 0xffff
    bound_new = (gm.cpu() & 0x7fff)[st["keep"]]
    full = (1 << G) - 1
    for name, bound in (("gs_band_project", bound_old), ("gs_band_frontend", bound_new)):
        missing = int(((exact & ~bound & full) != 0).sum())
        report(f"band mask superset G={G} fy/fx={fy_over_fx}", entry=name, V=V, missing=missing,
               exact_bits=int(exact.bitwise_and(full).ne(0).sum()))
        assert missing == 0, (name, missing)


E2E = {"large": dict(seed=60, N=200_000, W=1297, H=840, deg=3, stress=False),
       "small": dict(seed=61, N=4000, W=333, H=197, deg=2, stress=True)}
# bound on a kernel's render-gradient error per element, as a fraction of the oracle's sum of term magnitudes of that
# element (tests/test_gpu_scale.py: check_band_backward's noise-normalised criterion)
RENDER_NOISE = 2e-5


def oracle_render(exp, colour, rays, W, H, bg, gi):
    """the oracle's render forward + backward of every tile row from its own stages and lists; colour [V,3]
    (precomputed SH) or the coefficients [V,3,n_sh] with rays [H,W,3] (per-pixel SH)"""
    img, nsp, fw = torch.zeros(H, W, 3), torch.zeros(H, W, dtype=torch.int32), torch.zeros(H, W)
    args = (exp["uv"], exp["opacity"].reshape(-1, 1).contiguous(), colour, exp["conic"], rays, exp["ranges"],
            exp["sorted"], bg)
    gs_oracle.render_tiles_cuda(*args, nsp, fw, img)
    V = exp["V"]
    shapes = (tuple(colour.shape), (V, 1), (V, 2), (V, 3))
    g = [torch.zeros(*sh) for sh in shapes]
    gs_oracle.render_tiles_backward_cuda(*args, nsp, fw, gi, *g)
    a = [torch.zeros(*sh) for sh in shapes]
    gs_oracle.render_tiles_backward_abs(*args, nsp, fw, gi, *a)
    return dict(image=img, nsp=nsp, fw=fw, g_rgb=g[0], g_opa=g[1], g_uv=g[2], g_conic=g[3], a_rgb=a[0], a_opa=a[1],
                a_uv=a[2], a_conic=a[3])


def leaf_r(sc, case, got_of, slab, a_slab, rows_ok, skip=()):
    """max r of the leaf gradients got_of(name) against ref64's VJP of the oracle's render gradients `slab`.  Envelope:
    the fp32 oracle chain's deviation from ref64 on the same slab, plus RENDER_NOISE times the render-gradient term
    magnitudes a_slab carried through the stage in absolute value (ref64_abs_vjp) -- the most a kernel's render
    gradients that pass check_band_backward can move each leaf gradient"""
    ref_g = ref64_stage(sc, slab, case.vis_g)["grad"]
    env = oracle_vjp(sc, case.st, slab)
    carried = ref64_abs_vjp(sc, a_slab, case.vis_g)
    rs = {}
    for k in ref_g:
        if k in skip:
            continue
        got = got_of(k)
        assert not got[case.st["culled"]].any(), k
        e = (env[k].double() - ref_g[k]).abs() + RENDER_NOISE * carried[k]
        rs[k] = r_measure(got[rows_ok], ref_g[k][rows_ok], e[rows_ok])
    return rs


@pytest.mark.parametrize("name", list(E2E))
def test_end_to_end_frames_on_general_cameras(name):
    from gaussian_splatting_amd import splat_cuda
    from gaussian_splatting_amd.splat_py.utils import compute_rays_in_world_frame

    from .helpers import noise_normalised_err, rel_err, scaled_err
    from .test_gpu_scale import check_band_backward
    a = E2E[name]
    sc = general_camera_scene(a["seed"], a["N"], a["W"], a["H"], deg=a["deg"], stress=a["stress"])
    W, H = sc.W, sc.H
    tag = f"general_camera end_to_end[{name}]"
    case = Case(sc, lists=True)
    exp = case.st   # the fp32 oracle stages and lists (cpu_expected_stages)
    V = exp["V"]
    gi = make_grad_image(W, H, seed=2)
    bg = torch.full((3,), 0.5)
    params = ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")
    ok = torch.ones(sc.g.xyz.shape[0], dtype=torch.bool)   # Gaussians fp32 and fp64 cull alike
    ok[case.vis_g[~case.agree_v]] = False

    def frame(aux, precompute=True):
        g, cam, T = to_device(sc, DEV)
        for k in params:
            if getattr(g, k) is not None:
                getattr(g, k).requires_grad_(True)
        out = fused.rasterize(g, T, cam, sc.near, sc.far, sc.pad, sc.mh, precompute, bg.to(DEV), return_aux=aux)
        return g, out

    # ---- the Python orchestration with its intermediates -------------------------------------------------------------
    g_aux, (image, mask, uv, aux) = frame(True)
    for k in ("conic", "opacity", "rgb"):
        aux[k].retain_grad()
    uv.retain_grad()
    image.backward(gi.to(DEV))
    assert torch.equal(mask.cpu(), exp["culled"])
    assert torch.equal(aux["tile_ranges"].cpu(), exp["ranges"]) and torch.equal(aux["sorted_gaussians"].cpu(), exp["sorted"])
    rgb_gpu = aux["rgb"].detach().cpu().contiguous()
    # (the SH colour hangs on the camera centre, formed in double on both sides by different algorithms: the last ulp
    # may differ -- checked here -- and the render check then takes the GPU's colours)
    assert (rgb_gpu - exp["rgb"]).abs().max() <= 2e-6 * max(1.0, float(exp["rgb"].abs().max()))
    rgb = exp["rgb"] if torch.equal(rgb_gpu, exp["rgb"]) else rgb_gpu
    ref = oracle_render(exp, rgb, torch.zeros(1, 1, 1), W, H, bg, gi)
    assert torch.equal(image.detach().cpu(), ref["image"])
    # num_splats_per_pixel / final_weight through the reference-signature entry point on the frame's own stages
    nsp, fw, img2 = torch.zeros(H, W, dtype=torch.int32, device=DEV), torch.zeros(H, W, device=DEV), torch.zeros(H, W, 3, device=DEV)
    splat_cuda.render_tiles_cuda(uv.detach(), aux["opacity"].detach(), aux["rgb"].detach(), aux["conic"].detach(),
                                 torch.zeros(1, 1, 1, device=DEV), aux["tile_ranges"], aux["sorted_gaussians"],
                                 bg.to(DEV), nsp, fw, img2)
    assert torch.equal(nsp.cpu(), ref["nsp"]) and torch.equal(fw.cpu(), ref["fw"]) and torch.equal(img2.cpu(), ref["image"])
    grads = dict(uv=uv.grad, conic=aux["conic"].grad, opacity_act=aux["opacity"].grad, rgb_render=aux["rgb"].grad)
    check_band_backward(tag + " render backward", grads, ref)
    slab = torch.cat([ref["g_rgb"], ref["g_opa"], ref["g_uv"], ref["g_conic"]], dim=1)
    a_slab = torch.cat([ref["a_rgb"], ref["a_opa"], ref["a_uv"], ref["a_conic"]], dim=1)
    leaf = lambda gg: (lambda k: getattr(gg, k).grad.cpu())
    check(f"{tag} leaf gradients, python orchestration", leaf_r(sc, case, leaf(g_aux), slab, a_slab, ok))

    # ---- the native frame with default policies (what bench.py times): its own render backward and slab, checked
    # element by element against ref64 with the same envelope (nothing of the other path enters it) -------------------
    g_nat, (image2, mask2, uv2) = frame(False)
    image2.backward(gi.to(DEV))
    assert torch.equal(image2.detach().cpu(), ref["image"]) and torch.equal(mask2.cpu(), exp["culled"])
    check(f"{tag} leaf gradients, native frame", leaf_r(sc, case, leaf(g_nat), slab, a_slab, ok))

    # ---- the per-pixel-SH path (colours from per-pixel view directions, rays from K and the pose) ---------------------
    g3, (image3, mask3, _) = frame(False, precompute=False)
    image3.backward(gi.to(DEV))
    assert torch.equal(mask3.cpu(), exp["culled"])
    keep = exp["keep"]
    coeffs = torch.cat((sc.g.rgb[keep].unsqueeze(2), sc.g.sh[keep]), dim=2).contiguous()
    rays = compute_rays_in_world_frame(sc.cam, sc.T).contiguous()
    ref3 = oracle_render(exp, coeffs, rays, W, H, bg, gi)
    d3 = (image3.detach().cpu() - ref3["image"]).abs().amax(dim=2)
    report(tag + " per-pixel SH vs oracle", max_abs=float(d3.max()), over_1e5=float((d3 > 1e-5).float().mean()))
    assert (d3 > 1e-5).float().mean() < 2e-3 and d3.max() < 5e-3
    # its coefficient gradients ARE render gradients (per-pixel rays): element by element against the oracle's, by the
    # criteria tests/test_gpu_parity.py holds this kernel to (the floor-free noise-normalised error is reported: the
    # kernel's batched matrix-core contraction deviates from the oracle by more than summation-order noise on some
    # elements of the large frame)
    for k, sl in (("rgb", slice(0, 1)), ("sh", slice(1, None))):
        got = getattr(g3, k).grad.cpu()
        assert not got[~keep].any(), k
        got = got[keep].reshape(V, 3, -1)
        want = ref3["g_rgb"][:, :, sl].reshape(V, 3, -1)
        err = dict(noise_normalised=noise_normalised_err(got, want, ref3["a_rgb"][:, :, sl].reshape(V, 3, -1)),
                   scaled=scaled_err(got, want), rel_floor_1e2=rel_err(got, want, 1e-2))
        report(tag + " per-pixel SH coefficient gradients vs oracle", tensor=k, **err)
        assert err["scaled"] < 1e-5 and err["rel_floor_1e2"] < 1e-4, (k, err)
    # ... and the geometry's through ref64 (the colour column of the slab is zero: the colour does not hang on xyz)
    z3 = torch.zeros(V, 3)
    slab3 = torch.cat([z3, ref3["g_opa"], ref3["g_uv"], ref3["g_conic"]], dim=1)
    a3 = torch.cat([z3, ref3["a_opa"], ref3["a_uv"], ref3["a_conic"]], dim=1)
    check(f"{tag} leaf gradients, per-pixel SH", leaf_r(sc, case, leaf(g3), slab3, a3, ok, skip=("rgb", "sh")))

    # ---- render_depth: the oracle's depth render on its own stages -----------------------------------------------------
    g4, cam4, T4 = to_device(sc, DEV)
    depth = fused.render_depth(g4, 0.2, T4, cam4, sc.near, sc.pad, sc.mh)
    exp_d = cpu_expected_stages(sc.g, sc.cam, sc.T, sc.near, 3.0e38, sc.pad, sc.mh)   # (the depth path has no far cull)
    want = torch.full((H, W, 1), -1.0)
    gs_oracle.render_depth_cuda(exp_d["xyz_c"], exp_d["uv"], exp_d["opacity"].reshape(-1, 1).contiguous(),
                                exp_d["conic"], exp_d["ranges"], exp_d["sorted"], 0.2, want)
    differs = (depth.cpu() - want).abs() > 1e-4 * want.abs().clamp(min=1.0)
    report(tag + " render_depth vs oracle", differing=float(differs.float().mean()), covered=float((want > 0).float().mean()))
    assert (want > 0).any() and differs.float().mean() < 1e-4
