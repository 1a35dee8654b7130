"""The per-pixel absolute uv gradient (gs_render_tiles_backward_slab_abs / k_render_bwd_abs, fused.rasterize(absgrad=
True)) against tests/absgrad_ref.py.

The rule: noise_measure(absgrad, absgrad_walk, abs_walk["g_uv"]) <= max(the fp32 restatement's measure, the fp32
oracle's measure of its signed g_uv on the same scene) + NOISE_MARGIN (2e-5, tests/test_gpu_scale.py).  Both
environments come from code that is not under test; the maximum because the signed and the absolute sum are bounded by
the same per-term errors and sample them differently.  absgrad / abs_walk is at least 1.2e-2 on every scene (measured
on the CPU, tests/test_absgrad_ref.py), so a kernel that returns |sum|, drops a tile or a factor misses by orders of
magnitude.  Rows of Gaussians no pixel uses are exactly zero.

What "equal" can mean where atomics meet: a Gaussian's row receives one atomic add per tile that flushes it, in the
order the tiles' workgroups happen to get there.  One or two addends onto a cleared word give the same bits in either
order; from three on the last bit may differ between two runs of the SAME kernel.  So bit-equality (compat against
exact, the slab of the new entry against the plain entry's) is asserted on the rows that at most two tiles name --
every row of the one-tile scenes -- and the other rows are held to 2e-6 of the largest value, the bound
tests/test_gpu_fused.py uses where "the atomics' summation order is the only difference".

Measured on an MI355X (kernel / restatement / oracle's signed g_uv): 2.7e-8 / 2.7e-8 / 2.7e-8 (partial_48x40) to
2.5e-6 / 1.0e-6 / 1.5e-6 (long_1100), 3.3e-4 all three in opaque_stack; the frame 1.47e-5 / 1.48e-5 / 1.47e-5 on all
three paths.  The controller's case: the fp64 norms of the symmetric Gaussian are 0.0029 signed and 1876 absolute, the
threshold 2.33; accumulated from uv.grad 0.0029, from uv_absgrad 1876.29."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.densify import DensifyConfig, DensityController
from gaussian_splatting_amd.splat_py.structs import Camera, Gaussians
from gaussian_splatting_amd.synthetic import DEFAULTS
from gaussian_splatting_amd.train_ops import Adam

from . import render_ref64 as R
from .absgrad_ref import absgrad_fp64, evaluate, noise_measure, scene_absgrad
from .helpers import report, scaled_err
from .test_gpu_render_ref64 import NOISE_MARGIN, check_gradients, frame_inputs, frame_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCENES = list(R.render_scenes())
ONE_TILE = ("faint_300", "opaque_stack", "long_1100")
ORDER_TOL = 2e-6
MODES = {"exact": _hip.GS_BACKWARD_EXACT, "compat": _hip.GS_BACKWARD_COMPAT}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def staged(name):
    """the scene on the device: records of gs_pack_splats and the forward of gs_render_tiles_packed"""
    sc = R.render_scenes()[name]
    ref = R.reference(name, 1, "fp32")
    d = lambda x: x.to(DEV).contiguous()
    uv, opa, conic, rgb = d(sc.uv), d(sc.opacity), d(sc.conic), d(R.scene_coeff(sc, 1))
    ranges, sorted_g, bg = d(sc.ranges), d(sc.sorted_g), d(sc.bg)
    W, H, V = sc.W, sc.H, sc.V
    nty = (H + 15) // 16
    packed = torch.empty(V, _hip.GS_PACKED_WIDTH, device=DEV)
    _hip.call("gs_pack_splats", _p(uv), _p(opa), _p(conic), _p(rgb), V, _p(packed), _hip.GS_F32, _stream())
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    fw = torch.zeros(H, W, device=DEV)
    img = torch.zeros(H, W, 3, device=DEV)
    rays = torch.zeros(1, 1, 3, device=DEV)
    _hip.call("gs_render_tiles_packed", _p(packed), _p(rgb), _p(rays), _p(ranges), _p(sorted_g), _p(bg), W, H, 1, 0, nty,
              _p(nsp), _p(fw), _p(img), _hip.GS_F32, None, _stream())
    return SimpleNamespace(sc=sc, packed=packed, rgb=rgb, ranges=ranges, sorted_g=sorted_g, bg=bg, nsp=nsp, fw=fw,
                           gi=d(ref.grad_image.float()), W=W, H=H, V=V, nty=nty)


def backward(s, mode, absgrad=True, ordered=False):
    """-> (slab [V, 9], absgrad [V, 2] or None) on the CPU; ordered: tile_order as the prologue leaves it"""
    slab = torch.zeros(s.V, 9, device=DEV)
    order = None
    if ordered:
        nt = ((s.W + 15) // 16) * s.nty
        order = torch.full((nt + 8,), -7, dtype=torch.int32, device=DEV)
        _hip.call("gs_render_backward_prologue", None, 0, None, _p(order), s.W, s.H, 0, s.nty, _stream())
    walk = (_p(s.packed), _p(s.rgb), _p(s.ranges), _p(s.sorted_g), _p(s.bg), _p(s.nsp), _p(s.fw), _p(s.gi), s.W, s.H, 0,
            s.nty, _p(slab), ctypes.c_int64(0), None, _p(order), None, None, None, None, MODES[mode])
    if not absgrad:
        _hip.call("gs_render_tiles_backward_slab", *walk, _stream())
        return slab.cpu(), None
    out = torch.zeros(s.V, 2, device=DEV)
    _hip.call("gs_render_tiles_backward_slab_abs", *walk, None, _p(out), _stream())
    return slab.cpu(), out.cpu()


def slab_dict(slab):
    return dict(g_rgb=slab[:, fused.SLAB_RGB], g_opacity=slab[:, fused.SLAB_OPACITY], g_uv=slab[:, fused.SLAB_UV],
                g_conic=slab[:, fused.SLAB_CONIC])


def few_tiles(sc):
    """rows that at most two tiles name: their sums do not depend on the order of the atomics"""
    return torch.bincount(sc.sorted_g.long(), minlength=sc.V) <= 2


def same_up_to_order(a, b, fixed):
    assert torch.equal(a[fixed], b[fixed])
    assert scaled_err(a, b) < ORDER_TOL


def held(e, got, vals, tag="kernel"):
    """the rule of the module docstring; -> the assertion, to run after the report"""
    ref = e["ref"]
    vals["restated"], vals["oracle_signed"] = e["measure_restated"], e["measure_oracle"]
    vals[tag] = noise_measure(got, e["absgrad"], ref.abs_walk["g_uv"])

    def verdict():
        assert vals[tag] <= max(e["measure_restated"], e["measure_oracle"]) + NOISE_MARGIN, vals
        assert not got[~ref.used].any()
        assert bool((got[ref.used] > 0).all())
    return verdict


@pytest.mark.parametrize("name", SCENES)
def test_kernel_absgrad_against_the_reference(name):
    """gs_pack_splats -> gs_render_tiles_packed -> gs_render_tiles_backward_slab_abs in exact mode; the nine sums next to
    it are the plain entry's"""
    e = scene_absgrad(name)
    s = staged(name)
    slab, got = backward(s, "exact")
    plain, _ = backward(s, "exact", absgrad=False)
    vals = {}
    verdict = held(e, got, vals)
    ref, orc = e["ref"], e["orc"]
    grads = check_gradients(vals, "walk", slab_dict(slab), orc, ref.grad_walk, ref.abs_walk, ref.used)
    report(f"absgrad_kernel[{name}]", **vals)
    verdict()
    grads()
    if name in ONE_TILE:
        assert torch.equal(slab, plain)
    else:
        same_up_to_order(slab, plain, few_tiles(s.sc))
    # |sum| <= sum | |, term by term the same products: the slab's own uv pair, up to its rounding
    assert bool((got.double() + NOISE_MARGIN * ref.abs_walk["g_uv"] >= slab[:, fused.SLAB_UV].double().abs()).all())


@pytest.mark.parametrize("name", [n for n, sc in R.render_scenes().items() if R.first_chunk(sc, R.FP32, 1)])
def test_compat_mode_is_exact_mode_within_the_first_chunk(name):
    s = staged(name)
    slab_e, abs_e = backward(s, "exact")
    slab_c, abs_c = backward(s, "compat")
    fixed = few_tiles(s.sc)
    same_up_to_order(abs_c, abs_e, fixed)
    same_up_to_order(slab_c, slab_e, fixed)


@pytest.mark.parametrize("name", ["partial_48x40", "long_1100"])
def test_tile_order_given(name):
    e = scene_absgrad(name)
    s = staged(name)
    slab, got = backward(s, "exact", ordered=True)
    vals = {}
    verdict = held(e, got, vals)
    report(f"absgrad_kernel_ordered[{name}]", **vals)
    verdict()
    same_up_to_order(slab, backward(s, "exact", absgrad=False)[0], few_tiles(s.sc))


def test_null_absgrad_buffer_is_refused():
    s = staged("partial_33x17")
    slab = torch.zeros(s.V, 9, device=DEV)
    args = (_p(s.packed), _p(s.rgb), _p(s.ranges), _p(s.sorted_g), _p(s.bg), _p(s.nsp), _p(s.fw), _p(s.gi), s.W, s.H, 0,
            s.nty, _p(slab), ctypes.c_int64(0), None, None, None, None, None, None, MODES["exact"], None, None, _stream())
    assert _hip.lib().gs_render_tiles_backward_slab_abs(*args) == _hip.GS_EINVAL
    torch.cuda.synchronize()
    assert not slab.any()


# ---- the frame ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frame_absgrad():
    sc, ref, orc = frame_reference()
    return evaluate(sc, ref, orc)


def run_frame(path, absgrad, grad_image, antialiased=False, twice=False):
    g, cam, T, bg = frame_inputs()
    for k in ("xyz", "rgb", "opacity", "scale", "quaternion"):
        getattr(g, k).requires_grad_(True)
    prev = fused.SEGMENTS, fused.DEPTH_CUT
    fused.SEGMENTS, fused.DEPTH_CUT = path == "segments", path == "depth_cut"
    fused.keep_last_slab(True)
    out = SimpleNamespace()
    try:
        cut_before = fused.counters().get("depth_cut_frames", 0)
        _hip.set_backward_mode("exact")
        res = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, absgrad=absgrad,
                              antialiased=antialiased, **DEFAULTS)
        out.image, out.uv = res[0].detach().cpu(), res[2].detach().cpu()
        if absgrad:
            assert len(res) == 4 and not res[3].requires_grad and res[3].dtype == torch.float32
            out.before = res[3].clone().cpu()
        res[0].backward(grad_image, retain_graph=twice)
        out.slab = fused.last_slab().cpu()
        if absgrad:
            out.absgrad = res[3].clone().cpu()
            if twice:
                res[0].backward(grad_image)
                out.again = res[3].clone().cpu()
        out.cut_frames = fused.counters().get("depth_cut_frames", 0) - cut_before
    finally:
        _hip.set_backward_mode("compat")
        fused.keep_last_slab(False)
        fused.SEGMENTS, fused.DEPTH_CUT = prev
    return out


@pytest.mark.parametrize("path", ["plain", "segments", "depth_cut"])
def test_frame_absgrad_against_the_reference(path):
    """tests/test_gpu_render_ref64.py's frame (12000 Gaussians on 70 x 45, lists of up to 4186 entries) through
    fused.rasterize(absgrad=True), each path pinned as that test pins it"""
    sc, ref, orc = frame_reference()
    e = frame_absgrad()
    assert float(ref.fragile.float().mean()) <= 0.02
    gi = ref.grad_image.float().to(DEV)
    f = run_frame(path, True, gi, twice=True)
    base = run_frame(path, False, gi)
    assert f.cut_frames == base.cut_frames == (1 if path == "depth_cut" else 0)
    assert torch.equal(f.image, base.image) and torch.equal(f.uv, base.uv) and torch.equal(f.uv, sc.uv)
    assert tuple(f.before.shape) == (sc.V, 2) and not f.before.any()
    vals = {"V": sc.V}
    verdict = held(e, f.absgrad, vals, "frame")
    grads = check_gradients(vals, "walk", dict(slab_dict(f.slab), image=f.image), orc, ref.grad_walk, ref.abs_walk,
                            ref.used)
    report(f"absgrad_frame[{path}]", **vals)
    verdict()
    grads()
    assert bool((f.absgrad.double() + NOISE_MARGIN * ref.abs_walk["g_uv"]
                 >= f.slab[:, fused.SLAB_UV].double().abs()).all())
    # the second backward overwrote: twice the sums would miss by the sums themselves
    assert scaled_err(f.again, f.absgrad) < ORDER_TOL
    assert torch.equal(f.again[few_tiles(sc)], f.absgrad[few_tiles(sc)])


def test_frame_absgrad_antialiased():
    sc, ref, orc = frame_reference()
    f = run_frame("plain", True, ref.grad_image.float().to(DEV), antialiased=True)
    assert tuple(f.absgrad.shape) == (sc.V, 2) and bool(torch.isfinite(f.absgrad).all()) and bool(f.absgrad.any())
    assert bool((f.absgrad.double() + NOISE_MARGIN * ref.abs_walk["g_uv"]
                 >= f.slab[:, fused.SLAB_UV].double().abs()).all())


def test_nothing_visible():
    g, cam, T, bg = frame_inputs()
    g.xyz[:, 2] = -5.0   # behind the camera
    g.xyz.requires_grad_(True)
    image, mask, uv, uv_absgrad = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, absgrad=True,
                                                  **DEFAULTS)
    assert tuple(uv.shape) == (0, 2) and tuple(uv_absgrad.shape) == (0, 2) and bool(mask.all())
    image.sum().backward()
    torch.cuda.synchronize()
    assert tuple(uv_absgrad.shape) == (0, 2)


# ---- the case the feature exists for ----------------------------------------------------------------------------------
def _hand_frame():
    """64 x 64, identity pose: Gaussian 0 isotropic, centred between four pixels, 4 px wide; five ordinary ones"""
    W = H = 64
    f = 60.0
    z = 5.0
    centre = [[(31.5 - 32) / f * z, (31.5 - 32) / f * z, z]]
    gen = torch.Generator().manual_seed(3)
    others = torch.cat([(torch.rand(5, 2, generator=gen) - 0.5) * 4.0, 4.0 + 4.0 * torch.rand(5, 1, generator=gen)], dim=1)
    xyz = torch.cat([torch.tensor(centre), others])
    n = xyz.shape[0]
    scale = torch.log(torch.cat([torch.full((1, 3), 4.0 * z / f), 0.05 + 0.1 * torch.rand(5, 3, generator=gen)]))
    quat = torch.cat([torch.tensor([[1.0, 0.0, 0.0, 0.0]]), torch.randn(5, 4, generator=gen)])
    opacity = torch.cat([torch.tensor([[0.5]]), torch.randn(5, 1, generator=gen)])
    rgb = (0.2 + 0.6 * torch.rand(n, 3, generator=gen)) / 0.28209479177387814
    d = lambda t: t.float().to(DEV).contiguous()
    g = Gaussians(d(xyz), d(rgb), d(opacity), d(scale), d(quat))
    cam = Camera(W, H, d(torch.tensor([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])))
    return g, cam, torch.eye(4, device=DEV), torch.zeros(3, device=DEV)


def _reference_norms(row):
    """the fp64 reference's K-scaled norms of row `row`, signed and absolute, under the loss image.sum()"""
    g, cam, T, bg = _hand_frame()
    W, H = cam.width, cam.height
    _, _, uv, aux = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, return_aux=True, **DEFAULTS)
    cpu = lambda x: x.detach().cpu().contiguous()
    V = uv.shape[0]
    sc = SimpleNamespace(W=W, H=H, V=V, uv=cpu(uv), conic=cpu(aux["conic"]), opacity=cpu(aux["opacity"]).reshape(V, 1),
                         coeff16=cpu(aux["rgb"]).reshape(V, 3, 1), rays=torch.zeros(H, W, 3),
                         grad_image=torch.ones(H, W, 3), bg=torch.zeros(3), sorted_g=cpu(aux["sorted_gaussians"]).int(),
                         ranges=cpu(aux["tile_ranges"]).int())
    ref = R.render_fp64(sc.uv, sc.opacity, R.scene_coeff(sc, 1), sc.conic, sc.rays, sc.ranges, sc.sorted_g, sc.bg, W, H,
                        R.FP32, sc.grad_image)
    ref.grad_image = sc.grad_image.double() * (~ref.fragile)[:, :, None]
    absgrad, signed = absgrad_fp64(sc, ref)
    K = cam.K.cpu().double()
    k = torch.stack([K[0, 0], K[1, 1]])
    return float((signed[row] * k).norm()), float((absgrad[row] * k).norm()), cpu(aux["vis_idx"])


@pytest.mark.parametrize("feed", ["uv.grad", "uv_absgrad"])
def test_symmetric_gaussian_is_densified_from_absgrad_only(feed):
    """under image.sum() the per-pixel gradients of Gaussian 0 cancel in uv.grad; with uv_grad_threshold between its two
    norms (their geometric mean, from the fp64 reference) the controller densifies it when fed uv_absgrad and not when
    fed uv.grad"""
    signed_norm, abs_norm, vis_idx = _reference_norms(0)
    assert int(vis_idx[0]) == 0 and abs_norm > 10 * signed_norm
    thr = (max(signed_norm, 1e-30) * abs_norm) ** 0.5
    g, cam, T, bg = _hand_frame()
    names = ("xyz", "quaternion", "scale", "opacity", "rgb")
    params = [getattr(g, k).requires_grad_(True) for k in names]
    opt = Adam([{"params": p, "lr": 1e-3} for p in params])
    cfg = DensifyConfig(use_fractional_densification=False, use_adaptive_fractional_densification=False,
                        uv_grad_threshold=thr, scale_norm_percentile=1.0, use_delete=False,
                        adaptive_control_start=0, adaptive_control_end=100)
    ctrl = DensityController(g, opt, cfg)
    image, culled, uv, uv_absgrad = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, absgrad=True,
                                                    **DEFAULTS)
    uv.retain_grad()
    image.sum().backward()
    assert not bool(culled[0])
    ctrl.accumulate(uv.grad if feed == "uv.grad" else uv_absgrad, culled, cam)
    norm = torch.norm(ctrl.uv_grad_accum / ctrl.grad_accum_count.clamp(min=1).unsqueeze(1), dim=1)
    densify = norm > thr                      # the controller's decision (densify.py: uv_norm > uv_split_val)
    n = g.xyz.shape[0]
    info = ctrl.adaptive_density_control(1)
    report(f"absgrad_densify[{feed}]", signed_norm=signed_norm, abs_norm=abs_norm, threshold=thr, accumulated=float(norm[0]))
    assert info == ctrl.last_info and info["cloned"] + info["split"] == int(densify.sum())
    assert info["n_before"] == n and info["n_after"] > n - 1 + int(densify.sum())
    assert bool(densify[0]) == (feed == "uv_absgrad")
