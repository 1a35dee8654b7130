"""The median-depth map: gs_render_median_depth / gs_median_depth_backward and fused.rasterize_median_depth against the
float64 reference of tests/median_ref.py (held to what this file needs by tests/test_median_depth_ref.py on the CPU).
The scenes keep their seeded, unsorted z: the kernels are held to the LIST-ORDER definition.

Rules
  forward    depth, alpha and transmittance torch.equal to gs_render_zalpha's; median_index equal to the reference's on
             every pixel that is neither fragile (render_ref64's) nor median-fragile (T_k within MEDIAN_MARGIN = 2^-17 of
             0.5); on EVERY pixel median_depth torch.equal to z[median_index] (0 with -1), and the reference's T in front
             of the chosen entry > 0.5 (1 - MEDIAN_MARGIN), its T behind it <= 0.5 (1 + MEDIAN_MARGIN) unless the entry
             is the reference's last contributor; nothing is written outside the image
  backward   noise_measure(kernel) <= noise_measure(fp32 restatement) + NOISE_MARGIN against the float64 index_add
             (only the order of the fp32 additions differs); rows no pixel selects exactly zero; the kernel ADDS
  frame      image / depth / alpha / culling_mask / uv torch.equal to rasterize_rgbd's; xyz.grad of a median-depth loss
             against the float64 R[2, :] grad_z by ref64.r_measure <= R_MAX, every other parameter gradient exactly zero

Every case leaves its figures in the parity report."""
import functools

import pytest
import torch

from gaussian_splatting_amd import _hip, fused, train_ops
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

from . import depth_alpha_ref as D
from . import median_ref as M
from . import render_ref64 as R
from .helpers import rel_err, report
from .pose_terms import pose_r, pose_reference
from .ref64 import r_measure
from .test_gpu_depth_alpha import calls_of, frame_case, frame_inputs, param_grads
from .test_gpu_render_ref64 import FRAME, NOISE_MARGIN, R_MAX, noise_measure

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCENES = list(R.render_scenes())
SHIFT = FRAME["shift"]
GUARD = 16          # rows of sentinel behind every output: a partial tile's pixels below the image would land there
SENTINEL = -7


# ---- 1. the forward kernel against the reference ------------------------------------------------------------------------
def kernel_run(sc):
    """the depth scene through gs_pack_splats, gs_render_tiles_packed (for num_splats_per_pixel), gs_render_zalpha and
    gs_render_median_depth, the latter into NaN / SENTINEL-filled outputs with GUARD more rows -> dict of CPU tensors"""
    c = lambda x: x.to(DEV).float().contiguous() if x.is_floating_point() else x.to(DEV).contiguous()
    V, W, H = sc.V, sc.W, sc.H
    nty = (H + 15) // 16
    s = _hip.current_stream()
    p = _hip.ptr
    uv, opacity, conic, rgb = c(sc.uv), c(sc.opacity), c(sc.conic), c(sc.coeff16[:, :, 0])
    ranges, sorted_g, bg = c(sc.ranges), c(sc.sorted_g), c(sc.bg)
    packed = torch.empty(V, 12, device=DEV)
    _hip.call("gs_pack_splats", p(uv), p(opacity), p(conic), p(rgb), V, p(packed), _hip.GS_F32, s)
    image = torch.zeros(H, W, 3, device=DEV)
    fw = torch.zeros(H, W, device=DEV)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    _hip.call("gs_render_tiles_packed", p(packed), p(rgb), None, p(ranges), p(sorted_g), p(bg), W, H, 1, 0, nty, p(nsp),
              p(fw), p(image), _hip.GS_F32, None, s)
    xyz_cam = torch.zeros(V, 3, device=DEV)
    xyz_cam[:, 2] = sc.z.to(DEV)
    nan = lambda rows=H: torch.full((rows, W), float("nan"), device=DEV)
    zd, za, zt = nan(), nan(), nan()
    _hip.call("gs_render_zalpha", p(packed), p(xyz_cam), p(ranges), p(sorted_g), p(nsp), W, H, 0, nty, p(zd), p(za), p(zt), s)
    md, depth, alpha, t_end = (nan(H + GUARD) for _ in range(4))
    mi = torch.full((H + GUARD, W), SENTINEL, dtype=torch.int32, device=DEV)
    _hip.call("gs_render_median_depth", p(packed), p(xyz_cam), p(ranges), p(sorted_g), p(nsp), W, H, 0, nty, p(md), p(mi),
              p(depth), p(alpha), p(t_end), s)
    out = dict(nsp=nsp.cpu(), zalpha=(zd.cpu(), za.cpu(), zt.cpu()))
    for k, x in (("median_depth", md), ("median_index", mi), ("depth", depth), ("alpha", alpha), ("t_end", t_end)):
        x = x.cpu()
        guard = x[H:]
        assert bool((guard == SENTINEL).all() if k == "median_index" else torch.isnan(guard).all()), k
        out[k] = x[:H]
    return out


def forward_verdict(sc, ref, got, tag):
    """the forward rules of the module docstring -> the figures"""
    for k, z in zip(("depth", "alpha", "t_end"), got["zalpha"]):
        assert bool(torch.isfinite(got[k]).all()), k              # every pixel of the frame is written
        assert torch.equal(got[k], z), k                          # the depth kernel's bits
    idx = got["median_index"].long()
    assert bool(((idx >= -1) & (idx < sc.V)).all())
    has = idx >= 0
    assert torch.equal(got["median_depth"][has], sc.z[idx[has]])  # on every pixel, fragile ones included
    assert bool((got["median_depth"][~has] == 0).all())
    assert torch.equal(has, got["alpha"] > 0)
    assert torch.equal(idx[ref.ok], ref.median_index[ref.ok])
    listed, front, behind = M.choice_check(sc, ref, idx)
    assert bool(listed.all()) and bool(front.all()) and bool(behind.all()), (tag, int((~front).sum()), int((~behind).sum()))
    vals = dict(fragile=float(ref.fragile.float().mean()), median_fragile=float(ref.median_fragile.float().mean()),
                differs_on_fragile=int((idx != ref.median_index).sum()), no_contributor=float((~has).float().mean()))
    report(tag, **vals)
    print(f"{tag}: {vals}")
    return vals


@pytest.mark.parametrize("name", SCENES)
def test_forward_kernel_against_the_reference(name):
    sc, ref = D.depth_scene(name), M.reference(name)
    got = kernel_run(sc)
    assert torch.equal(got["nsp"][~ref.fragile], ref.nsp[~ref.fragile])
    forward_verdict(sc, ref, got, f"median_depth_kernel[{name}]")


# ---- 2. constructed one-tile scenes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.constructed()))
def test_forward_kernel_on_constructed_lists(name):
    case, ref = M.constructed()[name], M.constructed_reference(name)
    sc = case.sc
    got = kernel_run(sc)
    forward_verdict(sc, ref, got, f"median_depth_constructed[{name}]")
    idx = got["median_index"].long()
    first = idx[:, :16]
    if case.expect is not None:    # one list position for the whole tile, whatever chunk it was staged in
        assert bool((first == int(case.order[case.expect])).all()), name
        assert bool((got["median_depth"][:, :16] == sc.z[case.order[case.expect]]).all())
    if name.startswith("crossing_at_"):
        assert int(got["nsp"].min()) == 300
    if name == "never_crosses":
        assert float(got["alpha"].max()) < 0.5
    if name == "nobody_reaches":
        assert bool((first == -1).any()) and bool((first >= 0).any()) and bool((idx[:, 16:] == -1).all())
        assert not got["median_depth"][idx < 0].any()
    if name == "saturates_early":
        assert int(got["nsp"].max()) < sc.V
        pos = torch.empty(sc.V, dtype=torch.long)
        pos[case.order] = torch.arange(sc.V)
        assert bool((pos[first] < got["nsp"][:, :16]).all())      # inside the walked prefix


# ---- 3. the backward kernel -------------------------------------------------------------------------------------------
def backward_run(index, grad, V, W, H, start=None):
    """gs_median_depth_backward of index [H, W] (any integer dtype) and grad [H, W] (None: NULL) into grad_z [V] that
    holds `start` (zeros) -> grad_z on the CPU"""
    g_z = torch.zeros(V, device=DEV) if start is None else start.to(DEV).float().clone()
    idx = index.to(DEV).int().contiguous()
    gm = None if grad is None else grad.to(DEV).float().contiguous()
    _hip.call("gs_median_depth_backward", _hip.ptr(idx), _hip.ptr(gm), W, H, 0, (H + 15) // 16, _hip.ptr(g_z),
              _hip.current_stream())
    return g_z.cpu()


@pytest.mark.parametrize("name", SCENES)
def test_backward_kernel_against_the_reference(name):
    sc, ref = D.depth_scene(name), M.reference(name)
    V, W, H = sc.V, sc.W, sc.H
    gm = ref.grad_median.float()
    got = backward_run(ref.median_index, gm, V, W, H)
    vals = dict(restatement=noise_measure(ref.rest.g_z, ref.grad_z, ref.abs_z),
                kernel=noise_measure(got, ref.grad_z, ref.abs_z))
    # the kernel adds: a pattern in grad_z is one more term of every selected row's sum and stays as it is elsewhere
    pattern = torch.randn(V, generator=torch.Generator().manual_seed(3))
    onto = backward_run(ref.median_index, gm, V, W, H, start=pattern)
    selected = torch.zeros(V, dtype=torch.bool)
    selected[ref.median_index[ref.median_index >= 0]] = True
    vals["kernel_onto_pattern"] = noise_measure(onto, pattern.double() + ref.grad_z, ref.abs_z + pattern.double().abs())
    report(f"median_depth_backward[{name}]", **vals)
    print(f"median_depth_backward[{name}]: {vals}")
    bound = vals["restatement"] + NOISE_MARGIN
    assert vals["kernel"] <= bound and vals["kernel_onto_pattern"] <= bound, vals
    assert not got[~selected].any() and not got[~ref.used].any()   # rows no pixel selects: exactly zero
    assert got[ref.used].abs().max() > 0
    assert torch.equal(onto[~selected], pattern[~selected])
    assert torch.equal(backward_run(ref.median_index, None, V, W, H, start=pattern), pattern)   # NULL: nothing to add


def test_backward_kernel_sums_a_patch_in_the_wave():
    """every pixel of a 16 x 16 map selects Gaussian 5 with gradient 1: four waves, one atomic of 64.0 each"""
    got = backward_run(torch.full((16, 16), 5), torch.ones(16, 16), 8, 16, 16)
    assert float(got[5]) == 256.0 and not got[torch.arange(8) != 5].any()
    # two Gaussians interleaved in every wave, -1 in between, an image that is no multiple of the tile
    W, H = 37, 21
    idx = (torch.arange(W * H).reshape(H, W) % 3) - 1
    got = backward_run(idx, torch.full((H, W), 0.5), 2, W, H)
    assert got.tolist() == [0.5 * int((idx == 0).sum()), 0.5 * int((idx == 1).sum())]


def test_kernel_entry_points_validate():
    """bad arguments are GS_EINVAL with a message, as for the sibling map entry points; empty lists give 0, -1, 0, 0, 1"""
    z = torch.zeros(4, device=DEV)
    zi = torch.zeros(4, dtype=torch.int32, device=DEV)
    lib, s = _hip.lib(), _hip.current_stream()
    p = _hip.ptr
    E = _hip.GS_EINVAL
    assert lib.gs_render_median_depth(None, None, None, None, None, 0, 16, 0, 1, p(z), p(zi), p(z), p(z), p(z), s) == E
    assert b"non-empty" in lib.gs_last_error()
    assert lib.gs_render_median_depth(None, None, p(z), None, p(z), 16, 16, 0, 2, p(z), p(zi), p(z), p(z), p(z), s) == E
    assert b"tile row" in lib.gs_last_error()
    assert lib.gs_render_median_depth(None, None, p(z), None, p(z), 16, 16, 0, 1, p(z), p(zi), None, p(z), p(z), s) == E
    assert b"render_median_depth: an output is NULL" in lib.gs_last_error()
    for md, mi in ((None, p(zi)), (p(z), None)):
        assert lib.gs_render_median_depth(None, None, p(z), None, p(z), 16, 16, 0, 1, md, mi, p(z), p(z), p(z), s) == E
        assert b"render_median_depth: an output is NULL" in lib.gs_last_error()
    assert lib.gs_render_median_depth(None, None, None, None, p(z), 16, 16, 0, 1, p(z), p(zi), p(z), p(z), p(z), s) == E
    assert lib.gs_median_depth_backward(p(zi), p(z), 0, 16, 0, 1, p(z), s) == E
    assert b"non-empty" in lib.gs_last_error()
    assert lib.gs_median_depth_backward(p(zi), p(z), 16, 16, 0, 2, p(z), s) == E
    assert b"tile row" in lib.gs_last_error()
    assert lib.gs_median_depth_backward(None, p(z), 16, 16, 0, 1, p(z), s) == E
    assert b"median_index is NULL" in lib.gs_last_error()
    assert lib.gs_median_depth_backward(p(zi), p(z), 16, 16, 0, 1, None, s) == E
    assert b"grad_z is NULL" in lib.gs_last_error()
    assert lib.gs_median_depth_backward(p(zi), None, 16, 16, 0, 1, None, s) == _hip.GS_OK     # nothing to add
    assert lib.gs_median_depth_backward(p(zi), p(z), 16, 16, 1, 1, None, s) == _hip.GS_OK     # no tile rows
    assert lib.gs_render_median_depth(None, None, p(z), None, p(z), 16, 16, 1, 1, p(z), p(zi), p(z), p(z), p(z), s) == _hip.GS_OK
    # empty lists, V == 0
    W, H = 33, 17
    ranges = torch.zeros(3 * 2 + 1, dtype=torch.int32, device=DEV)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    m, d, a, t = (torch.full((H, W), 7.0, device=DEV) for _ in range(4))
    i = torch.full((H, W), 7, dtype=torch.int32, device=DEV)
    e = torch.empty(0, device=DEV)
    _hip.call("gs_render_median_depth", p(e), p(e), p(ranges), p(e), p(nsp), W, H, 0, 2, p(m), p(i), p(d), p(a), p(t), s)
    assert not m.any() and not d.any() and not a.any() and bool((t == 1).all()) and bool((i == -1).all())
    gz = torch.ones(1, device=DEV)
    _hip.call("gs_median_depth_backward", p(i), p(m), W, H, 0, 2, p(gz), s)
    assert bool((gz == 1).all())


# ---- 4. the frame -----------------------------------------------------------------------------------------------------
def median_frame(g, T, cam, bg, **kw):
    return fused.rasterize_median_depth(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS, **kw)


@functools.lru_cache(maxsize=None)
def frame_reference_median(shift):
    """the median reference on the frame's own complete lists (tests/test_gpu_depth_alpha.py's frame_case: a return_aux
    frame of fused.rasterize) for a seeded grad_median; once per shift"""
    case = frame_case(shift)
    gen = torch.Generator().manual_seed(FRAME["seed"] + 5)
    gm = torch.randn(FRAME["H"], FRAME["W"], generator=gen)
    return M.reference_of(case.sc, gm, case.ref.fragile, case.ref.nsp)


@pytest.mark.parametrize("shift,kw", [(SHIFT, {}), (0.0, {}), (SHIFT, dict(antialiased=True)),
                                      (SHIFT, dict(camera_model="fisheye"))],
                         ids=["long_lists", "shift0", "antialiased", "fisheye"])
def test_frame_outputs(shift, kw):
    """image / culling_mask / uv bit-equal to fused.rasterize's, depth / alpha to rasterize_rgbd's; median_index in the
    dense numbering: a visible row or -1; on the plain frames against the reference on the frame's own lists"""
    g, cam, T, bg = frame_inputs(shift, grads=False)
    image, depth, alpha, md, mi, mask, uv = median_frame(g, T, cam, bg, **kw)
    want = fused.rasterize_rgbd(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS, **kw)
    plain = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS, **kw)
    assert torch.equal(image, plain[0]) and torch.equal(mask, plain[1]) and torch.equal(uv, plain[2])
    assert torch.equal(image, want[0]) and torch.equal(depth, want[1]) and torch.equal(alpha, want[2])
    assert torch.equal(mask, want[3]) and torch.equal(uv, want[4])
    H, W = FRAME["H"], FRAME["W"]
    assert mi.dtype == torch.int32 and tuple(mi.shape) == (H, W) and not mi.requires_grad
    assert md.dtype == torch.float32 and tuple(md.shape) == (H, W)
    mi, md, mask = mi.cpu().long(), md.cpu(), mask.cpu()
    has = mi >= 0
    assert bool(((mi >= -1) & (mi < FRAME["N"])).all()) and torch.equal(has, alpha.cpu() > 0)
    assert not mask[mi[has]].any()                                 # dense numbering: only rows the cull kept
    assert bool((md[~has] == 0).all()) and bool((md[has] > 0).all())
    if kw:
        return
    case, ref = frame_case(shift), frame_reference_median(shift)
    vis = torch.nonzero(~mask).flatten()
    assert vis.numel() == case.sc.V
    got_v = torch.full((FRAME["N"],), -1, dtype=torch.long)
    got_v[vis] = torch.arange(vis.numel())
    idx_v = torch.where(has, got_v[mi.clamp(min=0)], torch.full_like(mi, -1))   # back to the visible numbering
    assert torch.equal(idx_v[ref.ok], ref.median_index[ref.ok])
    assert torch.equal(md[has], case.sc.z[idx_v[has]])
    listed, front, behind = M.choice_check(case.sc, ref, idx_v)
    assert bool(listed.all()) and bool(front.all()) and bool(behind.all())
    vals = dict(fragile=float(ref.fragile.float().mean()), median_fragile=float(ref.median_fragile.float().mean()),
                differs_on_fragile=int((idx_v != ref.median_index).sum()))
    report(f"median_depth_frame[shift {shift}]", **vals)
    print(f"median_depth_frame[shift {shift}]: {vals}")
    assert vals["median_fragile"] <= 0.01


@pytest.mark.parametrize("loss", ["median", "all"])
def test_frame_gradients_and_launches(loss):
    """a loss on median_depth alone: one gs_median_depth_backward and no walk; xyz.grad against the float64
    R[2, :] grad_z, every other parameter gradient exactly zero.  A loss on all four maps: one launch of each"""
    case, ref = frame_case(SHIFT), frame_reference_median(SHIFT)
    H, W = FRAME["H"], FRAME["W"]
    g, cam, T, bg = frame_inputs(SHIFT)
    gm = ref.grad_median.float().to(DEV)
    gen = torch.Generator().manual_seed(31)
    others = [torch.randn(H, W, generator=gen).to(DEV), torch.randn(H, W, generator=gen).to(DEV),
              torch.randn(H, W, 3, generator=gen).to(DEV)]
    outs = {}

    def run():
        image, depth, alpha, md, mi, mask, uv = median_frame(g, T, cam, bg)
        outs.update(mask=mask, mi=mi)
        if loss == "median":
            torch.autograd.backward([md], [gm])
        else:
            torch.autograd.backward([md, depth, alpha, image], [gm] + others)

    calls = calls_of(run)
    assert "gs_render_zalpha" not in calls and len(calls["gs_render_median_depth"]) == 1
    assert len(calls["gs_median_depth_backward"]) == 1 and len(calls["gs_z_backward"]) == 1
    assert len(calls["gs_render_backward_prologue"]) == 1
    if loss == "all":
        assert len(calls["gs_render_zalpha_backward"]) == 1 and len(calls["gs_render_tiles_backward_slab"]) == 1
        for k, a in param_grads(g).items():
            assert bool(torch.isfinite(a).all()) and bool(a.any()), k
        return
    assert "gs_render_zalpha_backward" not in calls and "gs_render_tiles_backward_slab" not in calls
    grads = param_grads(g)
    for k in ("quaternion", "scale", "opacity", "rgb", "sh"):
        if k in grads:
            assert not grads[k].any(), k                           # the median depth moves z alone
    mask = outs["mask"].cpu()
    vis = torch.nonzero(~mask).flatten()
    xyz_grad = grads["xyz"].cpu()
    assert not xyz_grad[mask].any()
    row = T.detach().cpu()[2, :3]
    want = ref.grad_z[:, None] * row.double()[None, :]
    rest = ref.rest.g_z[:, None] * row[None, :]
    r = r_measure(xyz_grad[vis], want, (rest.double() - want).abs())
    report("median_depth_frame[loss median]", r_xyz=r, used=int(ref.used.sum()))
    print(f"median_depth_frame[loss median]: r_xyz = {r:.3g}")
    assert r <= R_MAX, r
    assert not xyz_grad[vis][~ref.used].any() and bool(xyz_grad[vis][ref.used].any())


def test_frame_image_only_loss_costs_no_map_backward():
    """a loss on the image alone: the parameter gradients of fused.rasterize (another order of the atomics, nothing
    else) and neither map backward"""
    w = torch.randn(FRAME["H"], FRAME["W"], 3, generator=torch.Generator().manual_seed(12)).to(DEV)
    g, cam, T, bg = frame_inputs(SHIFT)
    image, mask, uv = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
    (image * w).sum().backward()
    want = param_grads(g)
    g, cam, T, bg = frame_inputs(SHIFT)
    out = {}
    calls = calls_of(lambda: out.update(image=median_frame(g, T, cam, bg)[0]) or (out["image"] * w).sum().backward())
    assert torch.equal(out["image"].detach(), image.detach())
    assert "gs_median_depth_backward" not in calls and "gs_render_zalpha_backward" not in calls
    assert "gs_z_backward" not in calls and "gs_render_zalpha" not in calls
    assert len(calls["gs_render_median_depth"]) == 1 and len(calls["gs_render_tiles_backward_slab"]) == 1
    vals = {}
    for k, a in param_grads(g).items():
        vals[k] = rel_err(a, want[k])
        assert vals[k] < 1e-4, (k, vals[k])
    report("median_depth_frame_image_only", **vals)


def test_frame_with_nothing_visible():
    g, cam, T, bg = frame_inputs(0.0)
    image, depth, alpha, md, mi, mask, uv = fused.rasterize_median_depth(g, T, cam, 0.1, 0.2, 100, 3.0, True, bg)
    assert uv.shape[0] == 0 and bool(mask.all())
    assert not md.any() and bool((mi == -1).all()) and not depth.any() and not alpha.any()
    (md.sum() + depth.sum() + alpha.sum() + image.sum()).backward()
    for k, a in param_grads(g).items():
        assert not a.any(), k


def test_pose_gradient_of_a_median_depth_loss():
    """camera_T_world requires a gradient, loss on median_depth alone: the slab is zero, so T.grad is the direct term of
    z = T[2, 0:3] . xyz + T[2, 3] on the kept g_z (tests/pose_terms.py's reference on the kept slab adds zeros), pose_r
    with the z term's |t64| and |t32 - t64| in B and E, as the depth and distortion pose cases"""
    g, cam, T, bg = frame_inputs(SHIFT)
    T.requires_grad_(True)
    w = torch.randn(FRAME["H"], FRAME["W"], generator=torch.Generator().manual_seed(4)).to(DEV)
    fused.keep_last_slab(True)
    try:
        image, depth, alpha, md, mi, mask, uv = median_frame(g, T, cam, bg)
        (md * w).sum().backward()
        slab, g_z = fused.last_slab(), fused.last_grad_z()
    finally:
        fused.keep_last_slab(False)
    assert slab is not None and g_z is not None and not slab.any()
    vis = torch.nonzero(~mask.cpu()).flatten()
    c = lambda x: x.detach().cpu()
    xyz_v = c(g.xyz)[vis]
    ref, B, E = pose_reference(xyz_v, c(g.quaternion)[vis], c(g.scale)[vis], c(T), c(cam.K), c(slab))
    gz = c(g_z)
    t64 = torch.zeros(vis.numel(), 3, 4, dtype=torch.float64)
    t64[:, 2, :3] = gz.double()[:, None] * xyz_v.double()
    t64[:, 2, 3] = gz.double()
    t32 = torch.zeros(vis.numel(), 3, 4)
    t32[:, 2, :3] = gz[:, None] * xyz_v
    t32[:, 2, 3] = gz
    ref, B, E = ref + t64.sum(0), B + t64.abs().sum(0), E + (t32.double() - t64).abs().sum(0)
    assert T.grad is not None and tuple(T.grad.shape) == (4, 4) and bool(torch.isfinite(T.grad).all())
    assert not T.grad[3].any()
    r = pose_r(T.grad, ref, B, E)
    report("median_depth_pose[median loss]", r=r)
    print(f"median_depth_pose: r = {r:.3g}")
    assert r <= R_MAX, r
    assert bool(t64.sum(0)[2].abs().max() > 0)
    # the kept g_z is the scatter of w by the frame's own index
    sel = mi.cpu() >= 0
    got_v = torch.full((FRAME["N"],), -1, dtype=torch.long)
    got_v[vis] = torch.arange(vis.numel())
    want = torch.zeros(vis.numel(), dtype=torch.float64).index_add_(0, got_v[mi.cpu().long()[sel]], w.cpu().double()[sel])
    mag = torch.zeros(vis.numel(), dtype=torch.float64).index_add_(0, got_v[mi.cpu().long()[sel]],
                                                                   w.cpu().double()[sel].abs())
    assert noise_measure(gz, want, mag) <= NOISE_MARGIN


# ---- 5. use: the normal-consistency regulariser on the median depth ---------------------------------------------------
def test_normal_consistency_on_the_median_depth():
    g, cam, T = make_scene(3000, 64, 48, 0, seed=5, device=DEV)
    for k in ("xyz", "quaternion", "scale", "opacity", "rgb"):
        getattr(g, k).requires_grad_(True)
    bg = torch.zeros(3, device=DEV)
    kw = dict(use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
    image, depth, alpha, normal_map, mask, uv = fused.rasterize_normals(g, T, cam, **kw)
    _, depth2, alpha2, md, mi, _, _ = fused.rasterize_median_depth(g, T, cam, **kw)
    assert torch.equal(depth2, depth) and torch.equal(alpha2, alpha)
    valid = (mi >= 0).float()
    loss = train_ops.normal_consistency_loss(normal_map, md, alpha, cam, depth_alpha=valid)
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    loss.backward()
    for k in ("xyz", "quaternion"):
        a = getattr(g, k).grad
        assert a is not None and bool(torch.isfinite(a).all()) and bool(a.any()), k
    # the default is the call as it was
    a = train_ops.normal_consistency_loss(normal_map.detach(), depth.detach(), alpha.detach(), cam)
    b = train_ops.normal_consistency_loss(normal_map.detach(), depth.detach(), alpha.detach(), cam, depth_alpha=None)
    n_d = fused.depth_to_normal(depth.detach(), alpha.detach(), cam)
    ok = (n_d != 0).any(dim=2)
    per = alpha.detach() - (normal_map.detach() * n_d).sum(dim=2)
    c = torch.where(ok, per, torch.zeros_like(per)).sum() / ok.sum().clamp(min=1)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_guards_raise_before_anything_is_enqueued():
    g, cam, T, bg = frame_inputs(0.0, grads=False)
    args = (g, T, cam, DEFAULTS["near_thresh"], DEFAULTS["far_thresh"], DEFAULTS["cull_mask_padding"], DEFAULTS["mh_dist"])
    sh = torch.zeros(FRAME["N"], 3, 3, device=DEV)
    g_sh = type(g)(g.xyz, g.rgb, g.opacity, g.scale, g.quaternion, sh)
    bad = [
        ("tile_rows", lambda: fused.rasterize_median_depth(*args, True, bg, tile_rows=(0, 2))),
        ("return_aux", lambda: fused.rasterize_median_depth(*args, True, bg, return_aux=True)),
        ("slab_sync", lambda: fused.rasterize_median_depth(*args, True, bg, slab_sync=lambda flat: None)),
        ("frame_hook", lambda: fused.rasterize_median_depth(*args, True, bg, frame_hook=lambda d: None)),
        ("adam_plan", lambda: fused.rasterize_median_depth(*args, True, bg, adam_plan=object())),
        ("per-pixel SH", lambda: fused.rasterize_median_depth(g_sh, *args[1:], False, bg)),
    ]
    for words, call in bad:
        _hip.enable_timing(True)
        try:
            with pytest.raises(RuntimeError, match=words):
                call()
            assert not _hip.collect_timing(), words   # no entry point was called
        finally:
            _hip.enable_timing(False)
