"""tests/render_ref64.py (the plain float64 compositing reference) against the CPU oracle's render kernels, on the
scenes the GPU kernels are then held to (tests/test_gpu_render_ref64.py).  What each scene is aimed at:

  partial_48x40, partial_48x40_black, partial_33x17   partial tiles right and bottom (33x17: one pixel wide / high),
                                                      empty tiles, tiles with a single entry; background 0.5 and 0
  strip_70x13                                         a frame one tile high
  faint_300          one tile, 300 faint splats: every pixel walks several LDS chunks, the last one partial
  opaque_stack       one tile, 70 near-opaque splats (opacity up to 0.98): every pixel stops early, at entries 9 to 12,
                     and the list continues with splats nobody reaches
  long_1100          one tile, 1100 entries: past the reference backward's first chunk, exact mode only
  edge_cases_32x16   Gaussians centred on a pixel (m = 0 there), a needle (correlation 0.995), Gaussians on the border
                     of two tiles that both lists name

Each with 1, 4, 9 and 16 colour coefficients (per-pixel SH on unit rays)."""
import pytest
import torch

from . import render_ref64 as R
from .helpers import scaled_err

SCENES = list(R.render_scenes())
N_SH = (1, 4, 9, 16)
# measured here: the largest scaled_err between the reference (FP64 settings) and the fp64 oracle over every scene,
# coefficient count and quantity is 1.8e-13 (opaque_stack: 1 / (1 - alpha) up to 50 amplifies the rounding of the
# weights); the other scenes stay below 3.1e-14.  Asserted: 10x that.
FP64_BOUND = 1.8e-12
# fp32 oracle against the reference (FP32 settings), largest absolute difference over every scene and coefficient
# count, measured here: image 8.5e-7 (long_1100), final weight 4.7e-7 (long_1100; 4.6e-8 in opaque_stack, whose
# final weights are 1.3e-3 at most).  Asserted: 10x each.
IMAGE_ABS = 8.5e-6
FW_ABS = 4.7e-6


def oracle():
    from oracle import gs_oracle
    gs_oracle.set_modes(0, 0)
    gs_oracle.set_sh_band1_mode(0)
    return gs_oracle


def oracle_run(sc, n_sh, dtype, grad_image, exact=True):
    orc = oracle()
    try:
        orc.set_backward_exact(int(exact))
        return R.run_module(orc, "cpu", sc, n_sh, dtype, grad_image)
    finally:
        orc.set_backward_exact(0)


def oracle_contrib(sc, n_sh):
    orc = oracle()
    img, fw = torch.zeros(sc.H, sc.W, 3), torch.zeros(sc.H, sc.W)
    nsp = torch.zeros(sc.H, sc.W, dtype=torch.int32)
    rays = sc.rays if n_sh > 1 else torch.zeros(1, 1, 1)
    return orc.render_tiles_with_contrib_count(sc.uv, sc.opacity, R.scene_coeff(sc, n_sh), sc.conic, rays, sc.ranges,
                                               sc.sorted_g, sc.bg, nsp, fw, img)


def test_scenes_hold_what_they_are_aimed_at():
    sc = R.render_scenes()
    lens = lambda name: (sc[name].ranges[1:] - sc[name].ranges[:-1]).tolist()
    for name in ("partial_48x40", "partial_33x17", "strip_70x13"):
        assert 1 in lens(name), name
    assert 0 in lens("partial_48x40") and 0 in lens("partial_48x40_black")
    assert len(lens("strip_70x13")) == 5 and len(lens("partial_33x17")) == 6 and len(lens("partial_48x40")) == 9
    assert R.max_list(sc["long_1100"]) > 960 and sc["long_1100"].exact_only
    assert {float(s.bg[0]) for s in sc.values()} == {0.0, 0.5}
    # every pixel of faint_300 walks the whole list, every pixel of opaque_stack stops early, at different entries
    for st in ("fp64", "fp32"):
        assert int(R.reference("faint_300", 1, st).nsp.min()) == 300
        nsp = R.reference("opaque_stack", 1, st).nsp
        assert int(nsp.max()) < 20 and nsp.unique().numel() >= 3
    # a pixel on a Gaussian's centre: one contributor fewer than entries walked, in the float64 settings too
    e = sc["edge_cases_32x16"]
    ref = R.reference("edge_cases_32x16", 1, "fp64")
    assert ref.nsp[7, 5] == 8 and ref.nsp[3, 20] == 6 and ref.nsp[8, 16] == 6
    both = set(e.sorted_g[:e.ranges[1]].tolist()) & set(e.sorted_g[e.ranges[1]:].tolist())
    assert len(both) >= 3
    # skipped entries trail the last contributor at a good share of the fp32 pixels (render_ref64: grad_walk)
    assert float((R.reference("partial_48x40", 1, "fp32").scale != 1).float().mean()) > 0.3


@pytest.mark.parametrize("n_sh", N_SH)
@pytest.mark.parametrize("name", SCENES)
def test_reference_equals_the_fp64_oracle(name, n_sh):
    """exact mode: image, num_splats, final weight and the four gradients.  Measured max scaled_err 1.8e-13
    (opaque_stack), 3.1e-14 elsewhere; asserted 10x the former.  With the FP64 settings nothing is skipped, so the
    reference's walk gradient is its true derivative."""
    sc = R.render_scenes()[name]
    ref = R.reference(name, n_sh, "fp64")
    got = oracle_run(sc, n_sh, torch.float64, ref.grad_image)
    assert torch.equal(got["nsp"], ref.nsp)
    assert bool((ref.scale == 1).all())
    for k in R.GRAD_KEYS:
        assert torch.equal(ref.grad[k], ref.grad_walk[k]) or scaled_err(ref.grad_walk[k], ref.grad[k]) < 1e-15
    for k, want in [("image", ref.image), ("fw", ref.fw)] + [(k, ref.grad[k]) for k in R.GRAD_KEYS]:
        assert want.abs().max() > 0
        assert scaled_err(got[k], want) < FP64_BOUND, (k, scaled_err(got[k], want))


# the scenes whose lists fit the reference's fp64 first chunk (320 / 160 / 128 / 64 entries with 1 / 4 / 9 / 16
# coefficients): the cases of the GPU test's compat-mode comparison
FIRST_CHUNK_CASES = [(name, n_sh) for name, sc in R.render_scenes().items() for n_sh in N_SH
                     if R.first_chunk(sc, R.FP64, n_sh)]


def test_first_chunk_cases():
    names = {n_sh: {name for name, k in FIRST_CHUNK_CASES if k == n_sh} for n_sh in N_SH}
    assert "long_1100" not in names[1] and "faint_300" in names[1] and "faint_300" not in names[4]
    assert all(len(names[n_sh]) >= 5 for n_sh in N_SH)


@pytest.mark.parametrize("name,n_sh", FIRST_CHUNK_CASES)
def test_compat_mode_is_exact_mode_within_the_first_chunk(name, n_sh):
    """the fp64 oracle's two backward modes on every scene whose lists fit the reference's first chunk: the same
    terms, which licenses the compat-mode comparison on the GPU"""
    sc = R.render_scenes()[name]
    gi = R.reference(name, n_sh, "fp64").grad_image
    a, b = oracle_run(sc, n_sh, torch.float64, gi, exact=True), oracle_run(sc, n_sh, torch.float64, gi, exact=False)
    for k in R.GRAD_KEYS:   # the same terms; the oracle adds the tiles' sums in whatever order its threads finish
        assert scaled_err(a[k], b[k]) < 1e-14, k


@pytest.mark.parametrize("n_sh", N_SH)
@pytest.mark.parametrize("name", SCENES)
def test_fp32_oracle_takes_the_reference_decisions(name, n_sh):
    """FP32 settings against the fp32 oracle on the non-fragile pixels: num_splats and the count of contributors
    equal, the image within 8.5e-6 and the final weight within 4.7e-6 (10x the measured 8.5e-7 and 4.7e-7).  Measured flipped pixels
    over all scenes at margin 0: none -- see MARGIN."""
    sc = R.render_scenes()[name]
    ref = R.reference(name, n_sh, "fp32")
    got = oracle_run(sc, n_sh, torch.float32, ref.grad_image)
    ok = ~ref.fragile
    assert torch.equal(got["nsp"][ok], ref.nsp[ok])
    assert torch.equal(oracle_contrib(sc, n_sh)[ok], ref.contrib[ok])
    assert float((got["image"].double() - ref.image)[ok].abs().max()) < IMAGE_ABS
    assert float((got["fw"].double() - ref.fw)[ok].abs().max()) < FW_ABS


@pytest.mark.parametrize("st", ("fp64", "fp32"))
@pytest.mark.parametrize("name", SCENES)
def test_fragile_pixels_are_few(name, st):
    """at most 2 % of each scene's pixels (measured: none in any scene at MARGIN = 2^-21; 2^-19 made 0.4 % to 9 % of
    opaque_stack's pixels fragile, all of which cross 0.9999)"""
    for n_sh in N_SH:
        ref = R.reference(name, n_sh, st)
        assert float(ref.fragile.float().mean()) <= 0.02
        assert not ref.grad_image[ref.fragile].any()


def test_margin_is_no_smaller_than_the_scenes_need():
    """the decisions of the fp32 oracle and of the reference on every pixel, fragile or not: none flips on these scenes
    (measured), so the smallest margin they need is 0 and MARGIN (2^-21, 8 ulp of an fp32 A at 0.9999) is a constant
    chosen from the number format, not a measured one; while nothing flips this test says no more than 0 <= MARGIN.
    It is kept for the day a scene is added: a pixel that flips must then lie within MARGIN of a threshold"""
    worst = 0.0
    for name, sc in R.render_scenes().items():
        for n_sh in (1, 16):
            ref = R.reference(name, n_sh, "fp32")
            got = oracle_run(sc, n_sh, torch.float32, ref.grad_image)
            flipped = (got["nsp"] != ref.nsp) | (oracle_contrib(sc, n_sh) != ref.contrib)
            flipped |= (got["image"].double() - ref.image).abs().amax(dim=2) > IMAGE_ABS
            if flipped.any():
                worst = max(worst, float(ref.closeness[flipped].max()))
    assert worst <= R.MARGIN


def _gradcheck_scene():
    """two tiles (32 x 16): an opaque pair in front that stops the pixels under it, a faint entry that stays below
    1/255 at most pixels, and two ordinary ones behind"""
    uv = torch.tensor([[6.3, 7.4], [7.1, 8.2], [6.6, 6.9], [18.4, 5.3], [15.2, 9.7], [25.6, 11.3]], dtype=torch.float64)
    conic = torch.tensor([[300.0, 3.0, 280.0], [320.0, -4.0, 300.0], [280.0, 1.0, 310.0], [9.0, 1.0, 7.0], [30.0, 5.0, 25.0],
                          [6.0, -2.0, 8.0]], dtype=torch.float64)
    opacity = torch.tensor([[0.985], [0.985], [0.985], [0.01], [0.6], [0.8]], dtype=torch.float64)
    coeff = torch.linspace(0.2, 2.9, 6 * 3 * 4, dtype=torch.float64).reshape(6, 3, 4).sin().abs()
    gen = torch.Generator().manual_seed(5)
    rays = torch.randn(16, 32, 3, generator=gen, dtype=torch.float64)
    rays = rays / rays.norm(dim=2, keepdim=True)
    ranges = torch.tensor([0, 6, 10], dtype=torch.int32)
    sorted_g = torch.tensor([0, 1, 2, 3, 4, 5, 3, 4, 5, 1], dtype=torch.int32)
    gi = torch.randn(16, 32, 3, generator=gen, dtype=torch.float64)
    return uv, opacity, coeff, conic, rays, ranges, sorted_g, torch.full((3,), 0.5, dtype=torch.float64), gi


@pytest.mark.parametrize("st", (R.FP32, R.FP64), ids=("fp32", "fp64"))
def test_reference_gradcheck(st):
    """torch.autograd.gradcheck of `grad` (the true derivative) against differences of sum(image * grad_image), on a
    scene with stopped pixels and, in the FP32 settings, below-threshold entries and pixels whose walk gradient is
    scaled; grad_image is zero on the pixels with a decision within 1e-5 of its threshold, so the differences (step
    1e-6) flip no decision that counts"""
    uv, opacity, coeff, conic, rays, ranges, sorted_g, bg, gi = _gradcheck_scene()
    ref = R.render_fp64(uv, opacity, coeff, conic, rays, ranges, sorted_g, bg, 32, 16, st, gi, margin=1e-5)
    keep = ~ref.fragile
    assert float(keep.float().mean()) > 0.8
    gi = gi * keep[:, :, None]   # the same pixels in every evaluation below (margin 0 there)
    assert bool((ref.nsp[:, :16][keep[:, :16]] < 6).any()) and bool((ref.nsp[:, :16] == 6).any())    # stopped and not
    if st is R.FP32:
        assert bool((ref.contrib < ref.nsp).any()) and bool((ref.scale != 1).any())

    def f(uv_, opacity_, coeff_, conic_):
        # the differentiable part of render_fp64, reached through its public result: loss = sum(image * gi), whose
        # gradient render_fp64 returns; gradcheck needs the graph, so rebuild the loss from the returned gradient
        ref = R.render_fp64(uv_, opacity_, coeff_, conic_, rays, ranges, sorted_g, bg, 32, 16, st, gi, margin=0.0)
        return _Loss.apply(uv_, opacity_, coeff_, conic_, (ref.image * gi).sum(), ref.grad)

    class _Loss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, uv_, opacity_, coeff_, conic_, loss, grad):
            ctx.grad = grad
            return loss.clone()

        @staticmethod
        def backward(ctx, go):
            g = ctx.grad
            return go * g["g_uv"], go * g["g_opacity"], go * g["g_rgb"], go * g["g_conic"], None, None

    ins = [x.clone().requires_grad_(True) for x in (uv, opacity, coeff, conic)]
    assert torch.autograd.gradcheck(f, ins, eps=1e-6, atol=1e-7, rtol=1e-5)
