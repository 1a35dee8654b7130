"""The antialiased opacity's reference (tests/antialias_ref.py) against known answers and autograd, the refusals of
fused.rasterize*(antialiased=True) that need no GPU, and the C ABI's three new entry points (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

from .antialias_ref import aa_terms, fold_slab, opacity_eff, opacity_eff_fp64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_preprocess_forward_mode", "gs_preprocess_backward_mode", "gs_pose_backward_mode")


def random_conics(V, seed):
    """conics of positive definite 2x2 matrices with sigmas spread over 0.03 .. 30 px, a fifth of them needles"""
    gen = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    s1 = 10.0 ** (-1.5 + 3.0 * u(V))
    s2 = torch.where(u(V) < 0.2, s1 * 10.0 ** (-3.0 * u(V)), 10.0 ** (-1.5 + 3.0 * u(V)))
    th = 3.141592653589793 * u(V)
    c, s = torch.cos(th), torch.sin(th)
    a = c * c * s1 * s1 + s * s * s2 * s2
    b = c * s * (s1 * s1 - s2 * s2)
    d = s * s * s1 * s1 + c * c * s2 * s2
    return torch.stack([a, 2 * b, d], dim=1)


def test_isotropic_splats_have_the_closed_form_factor():
    s2 = torch.tensor([1e-6, 0.01, 0.09, 0.25, 1.0, 1.44, 400.0], dtype=torch.float64)
    conic = torch.stack([s2, torch.zeros_like(s2), s2], dim=1)
    y = torch.full((len(s2), 1), 0.5, dtype=torch.float64)
    want = 0.5 * s2 / (s2 + 0.25)
    assert torch.allclose(opacity_eff_fp64(conic, y)[:, 0], want, rtol=1e-14, atol=0)
    assert torch.allclose(opacity_eff(conic, y, torch.float64)[:, 0], want, rtol=1e-14, atol=0)
    assert torch.allclose(opacity_eff(conic, y, torch.float32)[:, 0].double(), want, rtol=1e-6, atol=0)
    # the issue's table: sigma 0.3 px against 1.2 px, ratio of the integrated weights 2 pi sigma_d^2 opa_eff
    w = lambda v: (v + 0.25) * v / (v + 0.25)
    assert abs(w(0.09) / w(1.44) * 16 - 1.0) < 1e-12


def test_degenerate_conics_give_zero():
    conic = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 1.0], [1.0, 2.5, 1.0], [float("nan"), 0.0, 1.0], [-1.0, 0.0, 1.0]],
                         dtype=torch.float64)
    y = torch.full((5, 1), 0.7, dtype=torch.float64, requires_grad=True)
    c = conic.clone().requires_grad_(True)
    out = opacity_eff_fp64(c, y)
    assert not out.detach().any()
    out.sum().backward()
    # no NaN out of the unselected branch (the row whose input is itself a NaN aside)
    finite = torch.isfinite(conic).all(dim=1)
    assert not c.grad[finite].any() and not y.grad.any()
    for dtype in (torch.float32, torch.float64):
        assert not aa_terms(conic, dtype)["comp"].any()
        slab = torch.ones(5, 9, dtype=dtype)
        folded = fold_slab(conic, y, slab, dtype)
        assert not folded[:, 3].any() and torch.equal(folded[:, 6:9], slab[:, 6:9])


def test_gradcheck_of_the_fp64_function():
    # finite differences want a smooth neighbourhood: sigmas of 0.3 .. 3 px at aspect ratios up to 3 (the needles,
    # whose derivative 0.5 / comp is steep, are held to autograd in the next test)
    gen = torch.Generator().manual_seed(1)
    s1 = 0.3 * 10.0 ** torch.rand(24, generator=gen, dtype=torch.float64)
    s2 = s1 / (1.0 + 2.0 * torch.rand(24, generator=gen, dtype=torch.float64))
    th = 3.0 * torch.rand(24, generator=gen, dtype=torch.float64)
    c, s = torch.cos(th), torch.sin(th)
    conic = torch.stack([c * c * s1 * s1 + s * s * s2 * s2, 2 * c * s * (s1 * s1 - s2 * s2),
                         s * s * s1 * s1 + c * c * s2 * s2], dim=1).requires_grad_(True)
    y = torch.rand(24, 1, dtype=torch.float64, generator=gen).requires_grad_(True)
    assert torch.autograd.gradcheck(opacity_eff_fp64, (conic, y), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_fold_slab_is_the_vjp_of_the_fp64_function():
    V = 500
    conic = random_conics(V, 3).requires_grad_(True)
    gen = torch.Generator().manual_seed(4)
    y = torch.rand(V, 1, dtype=torch.float64, generator=gen).requires_grad_(True)
    slab = torch.randn(V, 9, dtype=torch.float64, generator=gen)
    out = torch.cat([opacity_eff_fp64(conic, y), conic], dim=1)
    g_conic, g_y = torch.autograd.grad(out, (conic, y), grad_outputs=slab[:, [3, 6, 7, 8]])
    folded = fold_slab(conic, y, slab, torch.float64)
    assert torch.equal(folded[:, [0, 1, 2, 4, 5]], slab[:, [0, 1, 2, 4, 5]])
    scale = lambda x: x.abs().max(dim=0, keepdim=True).values
    assert ((folded[:, 3:4] - g_y).abs() / scale(g_y)).max() < 1e-12
    assert ((folded[:, 6:9] - g_conic).abs() / (g_conic.abs() + 1e-9 * scale(g_conic))).max() < 1e-9
    # the fp32 evaluation is the same formula: it follows to fp32 accuracy where nothing cancels (round splats)
    round_ = random_conics(V, 5)
    round_[:, 1] = 0
    round_[:, 2] = round_[:, 0]
    f32 = fold_slab(round_, y, slab, torch.float32).double()
    f64 = fold_slab(round_, y, slab, torch.float64)
    assert ((f32 - f64).abs() / (f64.abs() + 1e-3 * scale(f64))).max() < 1e-4


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    lib = _hip.lib()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fwd_cut = list(lib.gs_preprocess_forward_cut.argtypes)
    bwd = list(lib.gs_preprocess_backward.argtypes)
    pose = list(lib.gs_pose_backward.argtypes)
    want = {"gs_preprocess_forward_mode": fwd_cut[:-1] + [I, P],      # + raster_mode before stream
            "gs_preprocess_backward_mode": bwd[:-1] + [I, P],
            "gs_pose_backward_mode": pose[:6] + [P] + pose[6:-1] + [I, P]}   # + opacity_act (the fold needs y), raster_mode
    assert fwd_cut[9:18] == [I, I, I, F, F, F, F, I, I]
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
        assert hasattr(raw, n), n
        assert n in _hip.EXPORTS
        fn = getattr(lib, n)
        assert fn.restype is I and list(fn.argtypes) == want[n], n
    assert lib.gs_abi_version() >= 14
    assert _hip.GS_RASTER_CLASSIC == 0 and _hip.GS_RASTER_ANTIALIASED == 1
    assert "sqrt(rho)" in src and "no epsilon" in src   # the arithmetic is documented where the entries are declared


def test_default_is_off_everywhere():
    import inspect
    for fn in (fused.rasterize, fused.rasterize_rgbd, fused.rasterize_features, fused.preprocess_forward,
               fused.preprocess_backward, fused.pose_backward):
        assert inspect.signature(fn).parameters["antialiased"].default is False, fn.__name__
    from gaussian_splatting_amd import sharded
    assert "antialiased" not in open(sharded.__file__).read()


def cpu_frame():
    g, cam, T = make_scene(50, 32, 32, 1, seed=1, device="cpu")
    return g, cam, T, torch.zeros(3)


@pytest.mark.parametrize("option", ["adam_plan", "tile_rows", "return_aux", "grad_sync", "slab_sync", "frame_hook"])
def test_antialiased_refuses_frame_options(option):
    g, cam, T, bg = cpu_frame()
    value = {"adam_plan": object(), "tile_rows": (0, 1), "return_aux": True}.get(option, lambda *a: None)
    match = "adam_plan" if option == "adam_plan" else "whole single-GPU frames"
    with pytest.raises(RuntimeError, match=match):
        fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, antialiased=True, **{option: value}, **DEFAULTS)
    with pytest.raises(RuntimeError, match=match):
        fused.rasterize_rgbd(g, T, cam, use_sh_precompute=True, background_rgb=bg, antialiased=True, **{option: value},
                             **DEFAULTS)
    with pytest.raises(RuntimeError, match=match):
        fused.rasterize_features(g, torch.zeros(50, 4), T, cam, use_sh_precompute=True, background_rgb=bg,
                                 antialiased=True, **{option: value}, **DEFAULTS)


def test_antialiased_refuses_per_pixel_sh_and_cpu_or_fp64_tensors():
    g, cam, T, bg = cpu_frame()
    with pytest.raises(RuntimeError, match="per-pixel SH"):
        fused.rasterize(g, T, cam, use_sh_precompute=False, background_rgb=bg, antialiased=True, **DEFAULTS)
    with pytest.raises(RuntimeError, match=r"rasterize\(antialiased=True\) needs float32 tensors on the GPU"):
        fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, antialiased=True, **DEFAULTS)
    with pytest.raises(RuntimeError, match="rasterize_rgbd needs float32 tensors on the GPU"):
        fused.rasterize_rgbd(g, T, cam, use_sh_precompute=True, background_rgb=bg, antialiased=True, **DEFAULTS)
    with pytest.raises(RuntimeError, match="rasterize_features needs float32 tensors on the GPU"):
        fused.rasterize_features(g, torch.zeros(50, 4), T, cam, use_sh_precompute=True, background_rgb=bg,
                                 antialiased=True, **DEFAULTS)
    g64, cam64, T64 = make_scene(50, 32, 32, 1, seed=1, device="cpu", dtype=torch.float64)
    with pytest.raises(RuntimeError, match="needs float32 tensors on the GPU"):
        fused.rasterize(g64, T64, cam64, use_sh_precompute=True, background_rgb=bg.double(), antialiased=True, **DEFAULTS)
