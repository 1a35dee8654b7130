"""The fused fp32 render kernels set their waves' priority -- k_render_fwd<float, 1> by launch position (the last
eighth of the grid), k_render_bwd<float, 1> by position in the list walk (high until two chunks remain) -- and nothing
else may change: on frames where only SOME workgroups take each branch the results are those of the six-node path.

Two frames.  (1) 96x80 = 30 tiles, grid 32: the last 1/8, 1/4 and 1/2 of the grid are 4, 8 and 16 workgroups, so both
sides of a launch-position guard run at each of these fractions; lists of a few hundred entries = two or more 256-entry forward chunks and
several 64-entry backward chunks.  (2) 736x720 = 46x45 = 2070 tiles with a mean list above 256: the smallest frame on
which the backward starts its tiles longest-first (>= 2048 tiles, mean list >= 256), so that its launch position is the
index into the tile order and not the tile number.

Scenes: synthetic.make_scene at SH degree 0 -- the colour is then the rgb parameter itself on both paths (with SH the
two paths form the camera centre by different algorithms and the colours differ in the last ulp) -- and with the
identity world->camera transform make_scene uses, so the per-Gaussian stage is exact on both: culling mask and uv are
bit-identical.  `sigma_scale` multiplies every sigma so that few Gaussians give long lists; the list lengths quoted at
the cases were counted on the CPU with the oracle's list builder (tests/helpers.oracle_stages).

The image.  The six-node path forms the opacity with torch.sigmoid, the fused frame with the library's own sigmoid (the
one the oracle restates as sigmoid_det); on the 96x80 frame 779 of the 4 000 opacities differ in the last ulp
(1.2e-7) and the two images by 2.4e-7 -- before this file's kernels set any priority, and with every other render
input (uv, conic, colour) bit-equal.  So the image is compared twice: as the six-node path stands, within the bound
tests/test_gpu_fused.py has for the same comparison, and torch.equal with the six-node path run on the library's
sigmoid (torch.sigmoid replaced by the oracle's sigmoid_det for that one forward), which is the statement that matters
here: same inputs, same bits.
Gradients: the tolerance of tests/test_gpu_fused.py's comparison of the same two paths (1e-4 of each tensor's scale)."""
import math

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.splat_py.rasterize import rasterize as rasterize_mirror
from gaussian_splatting_amd.synthetic import make_grad_image, make_scene

from .helpers import report, scaled_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
E2E_GRAD_TOL = 1e-4   # tests/test_gpu_fused.py: test_fused_matches_reference_shaped_path
PARAMS = ("xyz", "rgb", "opacity", "scale", "quaternion")
ARGS = (0.3, 500.0, 100, 3.0)   # near, far, cull padding, mh_dist


@pytest.fixture
def six_node_on_gpu():
    from gaussian_splatting_amd import backend, splat_cuda

    prev = backend._backend
    backend.use(splat_cuda)
    yield
    backend.use(prev)


def scene(N, W, H, seed, sigma_scale):
    g, cam, T = make_scene(N, W, H, 0, seed=seed, device=DEV)
    g.scale.add_(math.log(sigma_scale))
    return g, cam, T


def both_paths(N, W, H, seed, sigma_scale, bgval):
    bg = torch.full((3,), bgval, device=DEV)
    gi = make_grad_image(W, H, seed=seed + 9, device=DEV)
    outs = []
    for fn in (rasterize_mirror, fused.rasterize):
        g, cam, T = scene(N, W, H, seed, sigma_scale)
        for k in PARAMS:
            getattr(g, k).requires_grad_(True)
        img, mask, uv = fn(g, T, cam, *ARGS, True, bg)
        uv.retain_grad()
        img.backward(gi)
        outs.append((img.detach(), mask, uv.detach(), uv.grad, {k: getattr(g, k).grad for k in PARAMS}))
    return outs


def six_node_image_with_library_sigmoid(monkeypatch, N, W, H, seed, sigma_scale, bgval):
    """the six-node path's image with its opacities formed by the library's sigmoid (module docstring)"""
    from oracle import gs_oracle

    def sigmoid_det(x):
        return gs_oracle.sigmoid_det(x.detach().float().cpu().contiguous()).to(x.device)

    g, cam, T = scene(N, W, H, seed, sigma_scale)
    with monkeypatch.context() as m, torch.no_grad():
        m.setattr(torch, "sigmoid", sigmoid_det)
        img, _, _ = rasterize_mirror(g, T, cam, *ARGS, True, torch.full((3,), bgval, device=DEV))
    return img


def check(name, outs, img_same_opacity):
    (i0, m0, u0, gu0, p0), (i1, m1, u1, gu1, p1) = outs
    errs = {k: scaled_err(p1[k], p0[k]) for k in p0}
    errs["uv"] = scaled_err(gu1, gu0)
    diff = (i0 - i1).abs().amax(dim=2)
    report(name, image_max_diff=diff.max().item(), image_max_diff_same_opacity=(img_same_opacity - i1).abs().max().item(),
           uv_max_diff=(u0 - u1).abs().max().item(), grad_scaled_err=max(errs.values()))
    assert torch.equal(m0, m1)
    assert torch.equal(u0, u1)
    assert (diff > 1e-5).float().mean() < 2e-3 and diff.max() < 5e-3   # torch.sigmoid's last ulp
    assert torch.equal(img_same_opacity, i1)
    for k in p0:
        assert p1[k].shape == p0[k].shape
    assert max(errs.values()) < E2E_GRAD_TOL, errs


def list_stats(N, W, H, seed, sigma_scale):
    """tiles, list entries and the longest list of the frame, from the fused per-Gaussian stage and binning"""
    g, cam, T = scene(N, W, H, seed, sigma_scale)
    f = fused.preprocess_forward(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, T, cam.K, W, H, *ARGS, None,
                                 _hip.GS_SORT_PREFIX)
    lengths = (f.ranges[1:] - f.ranges[:-1])
    return int(lengths.numel()), int(f.S), int(lengths.max())


def test_plain_fused_path_some_workgroups_late(six_node_on_gpu, monkeypatch):
    """30 tiles (grid 32), 4 000 Gaussians, all inside the padded frustum, at make_scene's own sigma (0.5-6 px):
    15 818 list entries, lists of 446 ... 606 = two or three forward chunks and seven to ten backward chunks a tile"""
    N, W, H, seed, k = 4000, 96, 80, 3, 1.0
    nt, S, longest = list_stats(N, W, H, seed, k)
    assert nt == 30
    assert longest > 256 and S > 3 * 64 * nt   # more than one forward chunk; several backward chunks on average
    check("render_priority[96x80]", both_paths(N, W, H, seed, k, 0.5),
          six_node_image_with_library_sigmoid(monkeypatch, N, W, H, seed, k, 0.5))


def test_backward_with_the_tile_order_on(six_node_on_gpu, monkeypatch):
    """2070 tiles, 24 000 Gaussians at four times the sigma: 705 684 list entries, lists of 278 ... 408, mean 341
    (40 000 at twice the sigma average 196: below the 256 the order needs)"""
    N, W, H, seed, k = 24000, 736, 720, 4, 4.0
    nt, S, _ = list_stats(N, W, H, seed, k)
    # the conditions under which the fused frame orders the backward's tiles (fused.render_backward, frame_policy.h)
    assert nt == 2070 and nt >= 2048
    assert S >= fused.LPT_MIN_MEAN_LIST * nt and not fused.want_segments(S, nt)
    check("render_priority[736x720-ordered]", both_paths(N, W, H, seed, k, 0.0),
          six_node_image_with_library_sigmoid(monkeypatch, N, W, H, seed, k, 0.0))
