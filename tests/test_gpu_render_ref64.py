"""The HIP render kernels against tests/render_ref64.py, the plain float64 compositing reference written from the
formulas (the CPU oracle the other render tests use is a port of the same kernels; tests/test_render_ref64.py holds
the oracle to the same reference).  Scenes: render_ref64.render_scenes(), see tests/test_render_ref64.py.

float64 kernels (k_render_fwd_general<double> and k_render_bwd_ref): num_splats equal, image, final weight and the four gradients
within the scaled_err bound of the CPU test (1.8e-12); exact mode everywhere, compat mode where the lists fit the
reference's first chunk.

float32 kernels (k_render_fwd<float, 1> and k_render_bwd<float, 1> with one coefficient, k_render_fwd_general<float> and
k_render_bwd_sh with 4 / 9 / 16), non-fragile pixels only: num_splats equal; image and final weight
through ref64.r_measure with env = |fp32 oracle - reference| (bound 8, tests/test_gpu_general_cameras.py); gradients
through |got - ref| / abs_sum with the reference's own abs sums, where the kernel may exceed the fp32 oracle's value of
the same measure by 2e-5 (tests/test_gpu_scale.py's noise_normalised bound) and no more.  Two runs per case:
  true   grad_image only on the pixels whose walk is not scaled (render_ref64: scale == 1): the kernels' exact mode
         against the TRUE derivative `grad`
  walk   the whole grad_image against `grad_walk`: at the pixels whose last walked entry is a skipped one exact mode
         keeps the reference's weights, scaled by 1 / (1 - alpha_last); the reference models it
Measured on the CPU, fp32 oracle against the reference: 8.3e-6 at most (long_1100), 3.3e-4 in opaque_stack (final
weights of 1e-4 formed as 1 - A in fp32).  Against the true derivative on ALL pixels the oracle's measure is 1.6
(partial_48x40_black): exact mode is not the derivative there.
Measured on an MI355X (both backends, all scenes and coefficient counts):
  float64 kernels  scaled_err 1.7e-13 at most (opaque_stack, g_rgb), 3.0e-14 elsewhere; num_splats equal
  float32 kernels  r_image 0.28 to 0.83, r_fw 0.33 to 1.0; pixels with a scaled walk 0 to 57 %, fragile 0 %
                   walk: oracle 8.3e-6, kernel 1.1e-5 (long_1100); 3.3e-4 both in opaque_stack
                   true: oracle 6.7e-6, kernel 9.3e-6 (long_1100); 3.3e-4 both in opaque_stack
                   the kernel exceeds the oracle by 3.2e-6 at most (long_1100, g_rgb)

The frame's own path: one faint scene through fused.rasterize with fused.keep_last_slab(True) -- plain, with segments
forced (tests/test_gpu_segments.py) and with the depth cut on (tests/test_gpu_depth_cut.py) -- image and [V, 9] slab
against the reference fed the frame's own uv / conic / opacity / rgb and complete lists, same measures and bounds."""
import functools
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

from . import render_ref64 as R
from .helpers import report, scaled_err
from .ref64 import r_measure
from .test_render_ref64 import FP64_BOUND, oracle_run

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCENES = list(R.render_scenes())
N_SH = (1, 4, 9, 16)
R_MAX = 8.0          # tests/test_gpu_general_cameras.py
NOISE_MARGIN = 2e-5  # tests/test_gpu_scale.py: noise_normalised < 2e-5


def run_hip(mod, sc, n_sh, dtype, grad_image, mode):
    try:
        _hip.set_backward_mode(mode)
        return R.run_module(mod, DEV, sc, n_sh, dtype, grad_image)
    finally:
        _hip.set_backward_mode("compat")


# exact mode everywhere; compat mode where the lists fit the first chunk (beyond it compat mode is the reference's
# quirk, not a derivative: the oracle tests pin it)
FP64_CASES = [(name, n_sh, mode) for name, sc in R.render_scenes().items() for n_sh in N_SH
              for mode in ("exact", "compat") if mode == "exact" or R.first_chunk(sc, R.FP64, n_sh)]


@pytest.mark.parametrize("name,n_sh,mode", FP64_CASES)
def test_fp64_kernels_equal_the_reference(hip_backend, name, n_sh, mode):
    sc = R.render_scenes()[name]
    ref = R.reference(name, n_sh, "fp64")
    got = run_hip(hip_backend, sc, n_sh, torch.float64, ref.grad_image, mode)
    assert torch.equal(got["nsp"], ref.nsp)
    errs = {}
    for k, want in [("image", ref.image), ("fw", ref.fw)] + [(k, ref.grad[k]) for k in R.GRAD_KEYS]:
        errs[k] = scaled_err(got[k], want)
    report(f"render_ref64_fp64[{name}, n_sh {n_sh}, {mode}]", **errs)
    for k, e in errs.items():
        assert e < FP64_BOUND, (k, e)


def noise_measure(got, ref, abs_sum):
    """max |got - ref| / abs_sum over the elements somebody contributes to (0 if none)"""
    a = abs_sum.double().reshape(-1)
    d = (got.double().reshape(-1) - ref.double().reshape(-1)).abs()
    return float((d[a > 0] / a[a > 0]).max()) if bool((a > 0).any()) else 0.0


def forward_measures(got, orc, ref, ok):
    """r_measure of image and final weight on the pixels `ok`, env = |fp32 oracle - reference|"""
    vals = {}
    for k, want in (("image", ref.image), ("fw", ref.fw)):
        g, w, o = (x[ok].reshape(int(ok.sum()), -1) for x in (got[k].double(), want, orc[k].double()))
        vals[f"r_{k}"] = r_measure(g, w, o - w)
    return vals


def check_gradients(vals, tag, got, orc, want, abs_sum, used):
    """the issue's rule per gradient: kernel measure <= oracle measure + NOISE_MARGIN; unused rows exactly zero"""
    for k in R.GRAD_KEYS:
        vals[f"{tag}_oracle_{k}"] = noise_measure(orc[k], want[k], abs_sum[k])
        vals[f"{tag}_kernel_{k}"] = noise_measure(got[k], want[k], abs_sum[k])

    def verdict():
        for k in R.GRAD_KEYS:
            assert vals[f"{tag}_kernel_{k}"] <= vals[f"{tag}_oracle_{k}"] + NOISE_MARGIN, (tag, k, vals)
            assert not got[k][~used].any(), (tag, k)
            assert got[k][used].abs().max() > 0, (tag, k)
    return verdict


@pytest.mark.parametrize("n_sh", N_SH)
@pytest.mark.parametrize("name", SCENES)
def test_fp32_kernels_against_the_reference(hip_backend, name, n_sh):
    sc = R.render_scenes()[name]
    ref = R.reference(name, n_sh, "fp32")
    true = R.reference(name, n_sh, "fp32", True)
    ok = ~ref.fragile
    vals = {"scaled_pixels": float((ref.scale != 1).float().mean()), "fragile": float(ref.fragile.float().mean())}
    verdicts = []
    for tag, r, want, abs_sum in (("walk", ref, ref.grad_walk, ref.abs_walk), ("true", true, true.grad, true.abs)):
        orc = oracle_run(sc, n_sh, torch.float32, r.grad_image, exact=True)
        got = run_hip(hip_backend, sc, n_sh, torch.float32, r.grad_image, "exact")
        if tag == "walk":
            assert torch.equal(got["nsp"][ok], ref.nsp[ok])
            vals.update(forward_measures(got, orc, ref, ok))
        else:   # nothing scaled is left: the walk gradient is the true derivative
            assert all(scaled_err(true.grad_walk[k], true.grad[k]) < 1e-14 for k in R.GRAD_KEYS)
        verdicts.append(check_gradients(vals, tag, got, orc, want, abs_sum, r.used))
    report(f"render_ref64_fp32[{name}, n_sh {n_sh}]", **vals)
    assert vals["r_image"] <= R_MAX and vals["r_fw"] <= R_MAX, vals
    for v in verdicts:
        v()


# ---- the frame's own path -------------------------------------------------------------------------------------------
# 12000 Gaussians on 70 x 45 (partial tiles right and bottom), opacity logits lowered by 5.5: lists of up to 4186
# entries (33 segments, four times what the depth cut keeps) that most pixels walk to the end without saturating --
# a pixel that creeps up to 0.9999 in steps of 1e-6 is fragile (render_ref64.MARGIN), with a shift of -4 19 % are
FRAME = dict(N=12000, W=70, H=45, seed=7, shift=-5.5, bg=0.5)


def frame_inputs():
    c = FRAME
    g, cam, T = make_scene(c["N"], c["W"], c["H"], 0, seed=c["seed"], device=DEV)
    g.opacity.add_(c["shift"])
    return g, cam, T, torch.full((3,), c["bg"], device=DEV)


@functools.lru_cache(maxsize=None)
def frame_reference():
    """the frame's own uv / conic / opacity / rgb and complete lists (return_aux), the reference and the fp32 oracle
    on them; computed once for the three frame tests"""
    g, cam, T, bg = frame_inputs()
    W, H = FRAME["W"], FRAME["H"]
    _, _, uv, aux = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, return_aux=True, **DEFAULTS)
    cpu = lambda x: x.detach().cpu().contiguous()
    V = uv.shape[0]
    gen = torch.Generator().manual_seed(FRAME["seed"] + 1)
    sc = SimpleNamespace(name="frame", W=W, H=H, V=V, uv=cpu(uv), conic=cpu(aux["conic"]),
                         opacity=cpu(aux["opacity"]).reshape(V, 1), coeff16=cpu(aux["rgb"]).reshape(V, 3, 1),
                         rays=torch.zeros(H, W, 3), grad_image=torch.randn(H, W, 3, generator=gen),
                         bg=torch.full((3,), FRAME["bg"]), sorted_g=cpu(aux["sorted_gaussians"]).int(),
                         ranges=cpu(aux["tile_ranges"]).int())
    ref = R.render_fp64(sc.uv, sc.opacity, R.scene_coeff(sc, 1), sc.conic, sc.rays, sc.ranges, sc.sorted_g, sc.bg, W, H,
                        R.FP32, sc.grad_image)
    ref.grad_image = (sc.grad_image.double() * (~ref.fragile)[:, :, None]).contiguous()
    orc = oracle_run(sc, 1, torch.float32, ref.grad_image, exact=True)
    return sc, ref, orc


@pytest.mark.parametrize("path", ["plain", "segments", "depth_cut"])
def test_frame_slab_against_the_reference(path):
    """fused.rasterize (the packed entry points, gs_render_tiles_backward_slab) in exact mode: image through r_measure,
    the slab's columns (rgb 3 | opacity 1 | uv 2 | conic 3) against the reference's walk gradient by the rule of the
    fp32 kernel test; rows of Gaussians that no pixel uses exactly zero.  No separate `true` run as in the fp32 kernel
    test: on the pixels with scale == 1 the walk gradient IS the true derivative, and 96 % of this scene's pixels are
    scaled.  Each case pins both settings ("auto" would pick segments and the cut for these lists by itself): plain
    runs without either.  The cut's case asserts the frame counter and the repaired tiles; the frame module exposes
    no signal for segments, whose setting fused.rasterize hands to it on every call."""
    sc, ref, orc = frame_reference()
    assert float(ref.fragile.float().mean()) <= 0.02
    assert R.max_list(sc) > 2 * 1024 and int(ref.nsp.max()) > 2 * 1024   # many segments, beyond what the cut keeps
    g, cam, T, bg = frame_inputs()
    for k in ("xyz", "rgb", "opacity", "scale", "quaternion"):
        getattr(g, k).requires_grad_(True)
    prev = fused.SEGMENTS, fused.DEPTH_CUT
    fused.SEGMENTS, fused.DEPTH_CUT = path == "segments", path == "depth_cut"
    fused.keep_last_slab(True)
    try:
        fused.last_flags(clear=True)
        cut_before = fused.counters().get("depth_cut_frames", 0)
        _hip.set_backward_mode("exact")
        image, mask, uv = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
        image.backward(ref.grad_image.float().to(DEV))
        slab = fused.last_slab()
        assert slab is not None
        slab = slab.cpu()
        cut_frames = fused.counters().get("depth_cut_frames", 0) - cut_before
        flags = fused.last_flags()
    finally:
        _hip.set_backward_mode("compat")
        fused.keep_last_slab(False)
        fused.SEGMENTS, fused.DEPTH_CUT = prev
    assert cut_frames == (1 if path == "depth_cut" else 0)
    if path == "depth_cut":   # tiles ran out of the prefix the cut kept and were repaired from the complete list
        assert flags is not None and int(flags.sum()) > 0
    assert tuple(slab.shape) == (sc.V, 9) and torch.equal(uv.detach().cpu(), sc.uv)
    got = dict(image=image.detach().cpu(), g_rgb=slab[:, fused.SLAB_RGB], g_opacity=slab[:, fused.SLAB_OPACITY],
               g_uv=slab[:, fused.SLAB_UV], g_conic=slab[:, fused.SLAB_CONIC])
    ok = ~ref.fragile
    n = int(ok.sum())
    vals = {"V": sc.V, "max_list": R.max_list(sc), "scaled_pixels": float((ref.scale != 1).float().mean()),
            "fragile": float(ref.fragile.float().mean())}
    vals["r_image"] = r_measure(got["image"].double()[ok].reshape(n, -1), ref.image[ok].reshape(n, -1),
                                (orc["image"].double() - ref.image)[ok].reshape(n, -1))
    verdict = check_gradients(vals, "walk", got, orc, ref.grad_walk, ref.abs_walk, ref.used)
    report(f"render_ref64_frame[{path}]", **vals)
    assert vals["r_image"] <= R_MAX, vals
    verdict()
