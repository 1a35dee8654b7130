"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs.  Bit-exact for every fp32 forward quantity and all integer outputs (tile lists, ranges,
num_splats_per_pixel); gradients within 1e-4 of the tensor scale (atomic accumulation order is
the only source of difference).  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from gaussian_splatting_amd.splat_py.cuda_autograd_functions import (
    CameraPointProjection, ComputeConic, ComputeProjectionJacobian, ComputeSigmaWorld, PrecomputeRGBFromSH,
    RenderImage)
from gaussian_splatting_amd.splat_py.depth import render_depth
from gaussian_splatting_amd.splat_py.rasterize import frustum_culling_mask, rasterize
from gaussian_splatting_amd.splat_py.structs import Camera, Gaussians, Tiles
from gaussian_splatting_amd.splat_py.utils import compute_rays_in_world_frame, transform_points_torch
from gaussian_splatting_amd.synthetic import make_grad_image, make_scene

from .helpers import load, rel_err, scaled_err, scene6, scene_from_fixture, t

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4   # north_star: gradients within 1e-4 rel (element-wise, floor 1 % of max: helpers.rel_err)
DEV = "cuda"


def oracle():
    from oracle import gs_oracle
    gs_oracle.set_modes(0, 0)
    gs_oracle.set_sh_band1_mode(0)
    return gs_oracle


def cpu_stage_inputs(N, W, H, deg, seed, near=0.3, far=500.0, pad=100):
    """Runs the per-Gaussian part of the pipeline on the CPU oracle and returns everything the
    later stages consume (all CPU tensors)."""
    orc = oracle()
    g, cam, T = make_scene(N, W, H, deg, seed=seed)
    xyz_c = transform_points_torch(g.xyz, T)
    uv = torch.zeros(N, 2)
    orc.camera_projection_cuda(xyz_c, cam.K, uv)
    keep = ~frustum_culling_mask(xyz_c, uv, cam, near, far, pad)
    uv, xyz_c = uv[keep].contiguous(), xyz_c[keep].contiguous()
    V = uv.shape[0]
    sigma = torch.zeros(V, 3, 3)
    orc.compute_sigma_world_cuda(g.quaternion[keep].contiguous(), g.scale[keep].contiguous(), sigma)
    J = torch.zeros(V, 2, 3)
    orc.compute_projection_jacobian_cuda(xyz_c, cam.K, J)
    conic = torch.zeros(V, 3)
    orc.compute_conic_cuda(sigma, J, T, conic)
    opacity = torch.sigmoid(g.opacity[keep]).contiguous()
    d = dict(g=g, cam=cam, T=T, keep=keep, uv=uv, xyz_c=xyz_c, conic=conic, opacity=opacity,
             rgb=g.rgb[keep].contiguous(), xyz=g.xyz[keep].contiguous(), W=W, H=H, V=V)
    if g.sh is not None:
        d["sh_coeffs"] = torch.cat((g.rgb[keep].unsqueeze(2), g.sh[keep]), dim=2).contiguous()
    return d


# ---------------------------------------------------------------------------------------------------
# per-Gaussian kernels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_per_gaussian_forward_parity(hip_backend, dtype):
    orc = oracle()
    N = 20000
    g, cam, T = make_scene(N, 640, 480, 3, seed=1, dtype=dtype)
    T = T.clone()
    T[:3, :3] = torch.tensor([[0.9999, 0.0089, 0.0073], [-0.0106, 0.9568, 0.2905], [-0.0044, -0.2906, 0.9568]],
                             dtype=dtype)
    T[:3, 3] = torch.tensor([-0.3283, -1.9260, 2.9581], dtype=dtype)
    xyz_c = transform_points_torch(g.xyz, T)
    sh_coeffs = torch.cat((g.rgb.unsqueeze(2), g.sh), dim=2).contiguous()
    Tinv = torch.inverse(T).contiguous()

    def run(mod, dev):
        c = lambda x: x.to(dev).contiguous()
        out = {}
        out["uv"] = torch.zeros(N, 2, dtype=dtype, device=dev)
        mod.camera_projection_cuda(c(xyz_c), c(cam.K), out["uv"])
        out["sigma"] = torch.zeros(N, 3, 3, dtype=dtype, device=dev)
        mod.compute_sigma_world_cuda(c(g.quaternion), c(g.scale), out["sigma"])
        out["J"] = torch.zeros(N, 2, 3, dtype=dtype, device=dev)
        mod.compute_projection_jacobian_cuda(c(xyz_c), c(cam.K), out["J"])
        out["conic"] = torch.zeros(N, 3, dtype=dtype, device=dev)
        mod.compute_conic_cuda(out["sigma"], out["J"], c(T), out["conic"])
        for n_sh in (1, 4, 9, 16):
            co = c(sh_coeffs[:, :, :n_sh])
            out[f"rgb{n_sh}"] = torch.zeros(N, 3, dtype=dtype, device=dev)
            mod.precompute_rgb_from_sh_cuda(c(g.xyz), co, c(Tinv), out[f"rgb{n_sh}"])
        return {k: v.cpu() for k, v in out.items()}

    ref = run(orc, "cpu")
    got = run(hip_backend, DEV)
    for k in ref:
        if dtype == torch.float32:
            assert torch.equal(got[k], ref[k]), f"{k}: fp32 forward must be bit-identical"
        else:
            assert scaled_err(got[k], ref[k]) < 1e-13, k


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_per_gaussian_backward_parity(hip_backend, dtype):
    orc = oracle()
    N = 20000
    tol = 2e-5 if dtype == torch.float32 else 1e-12
    g, cam, T = make_scene(N, 640, 480, 3, seed=2, dtype=dtype)
    xyz_c = transform_points_torch(g.xyz, T)
    xyz_c[::7, 2] *= -1   # some points behind the camera: Q10
    gen = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dtype)
    g_uv, g_sigma, g_J, g_conic, g_rgb = rnd(N, 2), rnd(N, 3, 3), rnd(N, 2, 3), rnd(N, 3), rnd(N, 3)
    sigma = torch.zeros(N, 3, 3, dtype=dtype)
    orc.compute_sigma_world_cuda(g.quaternion, g.scale, sigma)
    J = torch.zeros(N, 2, 3, dtype=dtype)
    orc.compute_projection_jacobian_cuda(xyz_c, cam.K, J)
    Tinv = torch.inverse(T).contiguous()

    def run(mod, dev):
        c = lambda x: x.to(dev).contiguous()
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=dev)
        out = {}
        out["xyz_from_uv"] = z(N, 3)
        mod.camera_projection_backward_cuda(c(xyz_c), c(cam.K), c(g_uv), out["xyz_from_uv"])
        out["xyz_from_J"] = z(N, 3)
        mod.compute_projection_jacobian_backward_cuda(c(xyz_c), c(cam.K), c(g_J), out["xyz_from_J"])
        out["q"], out["scale"] = z(N, 4), z(N, 3)
        mod.compute_sigma_world_backward_cuda(c(g.quaternion), c(g.scale), c(g_sigma), out["q"], out["scale"])
        out["sigma"], out["J"] = z(N, 3, 3), z(N, 2, 3)
        mod.compute_conic_backward_cuda(c(sigma), c(J), c(T), c(g_conic), out["sigma"], out["J"])
        for n_sh in (1, 4, 9, 16):
            out[f"sh{n_sh}"] = z(N, 3, n_sh)
            mod.precompute_rgb_from_sh_backward_cuda(c(g.xyz), c(Tinv), c(g_rgb), out[f"sh{n_sh}"])
        return {k: v.cpu() for k, v in out.items()}

    ref = run(orc, "cpu")
    got = run(hip_backend, DEV)
    assert torch.equal(got["xyz_from_uv"][::7], torch.zeros_like(got["xyz_from_uv"][::7]))   # Q10
    for k in ref:
        assert scaled_err(got[k], ref[k]) < tol, f"{k}: {scaled_err(got[k], ref[k])}"


# ---------------------------------------------------------------------------------------------------
# tile binning + sort: exact
# ---------------------------------------------------------------------------------------------------
def test_tile_culling_reference_known_answer(hip_backend):
    """test/test_tile_culling.py:72-108 through the HIP path"""
    ka = load("ref_known_answers.npz")
    g, cam, T, _ = scene6(DEV)
    xyz_c = transform_points_torch(g.xyz, T)
    uv = CameraPointProjection.apply(xyz_c, cam.K)
    pad = 10
    mask = (xyz_c[:, 2] < 0.3) | (uv[:, 0] < -pad) | (uv[:, 0] > cam.width + pad) | (uv[:, 1] < -pad) | (
        uv[:, 1] > cam.height + pad)
    uv, xyz_c = uv[~mask].contiguous(), xyz_c[~mask].contiguous()
    s = ComputeSigmaWorld.apply(g.quaternion[~mask].contiguous(), g.scale[~mask].contiguous())
    J = ComputeProjectionJacobian.apply(xyz_c, cam.K)
    conic = ComputeConic.apply(s, J, T)
    sorted_g, ranges = hip_backend.get_sorted_gaussian_list(1024, uv, xyz_c, conic, 40, 30, 3.0)
    assert torch.equal(sorted_g.cpu(), t(ka["tile_culling_sorted"]))
    assert ranges.shape[0] == 1201


@pytest.mark.parametrize("N,W,H,seed", [(1000, 256, 256, 0), (30000, 640, 480, 4), (4000, 64, 48, 6)])
def test_tile_lists_bit_exact(hip_backend, N, W, H, seed):
    """tile assignment, per-tile ranges and depth order identical to the oracle; the third case
    packs ~1000+ Gaussians per tile (multi-pass LDS sort sizes)"""
    orc = oracle()
    d = cpu_stage_inputs(N, W, H, 0, seed)
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    ref_sorted, ref_ranges = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], ntx, nty, 3.0)
    got_sorted, got_ranges = hip_backend.get_sorted_gaussian_list(
        1024, d["uv"].to(DEV), d["xyz_c"].to(DEV), d["conic"].to(DEV), ntx, nty, 3.0)
    assert torch.equal(got_ranges.cpu(), ref_ranges)
    assert torch.equal(got_sorted.cpu(), ref_sorted)
    assert ref_sorted.numel() > N


def extreme_footprints(seed, W, H, n=600):
    """uv / depth / conic rows around the edges of the tile walk's arithmetic: conics from 1e-38 to 3e38, inf, NaN, zero
    and negative (axes beyond the range where the separable test applies, binning.hip: sat_separable), centres on tile
    boundaries, denormal, far outside the image, non-finite"""
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(-40, W + 40, n), rng.uniform(-40, H + 40, n)], 1).astype(np.float32)
    a, c = 10 ** rng.uniform(-2, 3, n), 10 ** rng.uniform(-2, 3, n)
    b = rng.uniform(-0.9, 0.9, n) * np.sqrt(a * c)
    conic = np.stack([a, 2 * b, c], 1).astype(np.float32)
    z = rng.uniform(0.5, 50, n).astype(np.float32)
    k = 0
    with np.errstate(all="ignore"):
        for v in (1e30, 1e33, 3e38, np.inf, np.nan, 1e-30, 1e-38, 0.0, -1.0):
            for row in ([v, 0.0, 1.0], [1.0, 0.0, v], [v, 0.0, v], [4.0, v, 4.0], [v, v, v]):
                conic[k] = row
                k += 1
        for u in (0.0, 16.0, 32.0, -16.0, 1e-40, -1e-40, 15.999999, 16.000002, 1e9, -1e9, np.inf, np.nan, float(W),
                  W - 1e-3):
            uv[k] = [u, 50.0]
            uv[k + 1] = [50.0, u]
            uv[k + 2], conic[k + 2] = [u, u], [0.05, 0.0, 0.05]
            k += 3
    xyz_c = np.stack([np.zeros(n), np.zeros(n), z], 1).astype(np.float32)
    return torch.from_numpy(uv), torch.from_numpy(xyz_c), torch.from_numpy(conic)


@pytest.mark.parametrize("seed,W,H,n", [(0, 256, 192, 600), (1, 640, 480, 600), (2, 50, 40, 600), (3, 50, 40, 4000),
                                         (4, 128, 96, 12000)])
def test_tile_lists_bit_exact_on_extreme_footprints(hip_backend, seed, W, H, n):
    """the tile walk's two forms of the separating-axis test (separable for finite, moderate axes; the reference's
    four-corner form otherwise) and its closed-form window give the oracle's lists on the rows where they could part
    (600 rows: the atomic-counter kernels with 16 lanes per Gaussian; 4000 and 12000: the LDS-histogram kernels with
    the column-hoisted walk)"""
    orc = oracle()
    uv, xyz_c, conic = extreme_footprints(seed, W, H, n)
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    ref_sorted, ref_ranges = orc.get_sorted_gaussian_list(1024, uv, xyz_c, conic, ntx, nty, 3.0)
    got_sorted, got_ranges = hip_backend.get_sorted_gaussian_list(1024, uv.to(DEV), xyz_c.to(DEV), conic.to(DEV), ntx, nty,
                                                                  3.0)
    assert torch.equal(got_ranges.cpu(), ref_ranges)
    assert torch.equal(got_sorted.cpu(), ref_sorted)
    assert ref_sorted.numel() > 600


def test_tile_lists_with_duplicate_depths(hip_backend):
    """ties in z: broken by ascending Gaussian index == the oracle's stable sort"""
    orc = oracle()
    d = cpu_stage_inputs(5000, 320, 240, 0, 8)
    d["xyz_c"][:, 2] = torch.round(d["xyz_c"][:, 2])   # many equal depths
    ref = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], 20, 15, 3.0)
    got = hip_backend.get_sorted_gaussian_list(1024, d["uv"].to(DEV), d["xyz_c"].to(DEV), d["conic"].to(DEV), 20,
                                               15, 3.0)
    assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])


def test_tile_lists_oversize_tile_falls_back_to_global_sort(hip_backend):
    """more instances in one tile than the LDS sort holds (8192)"""
    orc = oracle()
    gen = torch.Generator().manual_seed(3)
    V = 12000
    uv = torch.rand(V, 2, generator=gen) * 14 + 1       # all inside tile 0
    conic = torch.tensor([[1.0, 0.0, 1.0]]).repeat(V, 1).contiguous()
    xyz_c = torch.cat([torch.zeros(V, 2), 1 + 10 * torch.rand(V, 1, generator=gen)], dim=1).contiguous()
    ref = orc.get_sorted_gaussian_list(1024, uv, xyz_c, conic, 2, 2, 3.0)
    got = hip_backend.get_sorted_gaussian_list(1024, uv.to(DEV), xyz_c.to(DEV), conic.to(DEV), 2, 2, 3.0)
    assert int(ref[1][1]) >= V
    assert torch.equal(got[1].cpu(), ref[1]) and torch.equal(got[0].cpu(), ref[0])


@pytest.mark.parametrize("N,W,H", [(3000, 640, 480), (60000, 320, 240)])   # global-atomic path, LDS-histogram path
def test_tile_lists_with_screen_filling_gaussians(hip_backend, N, W, H):
    """Gaussians whose candidate window holds hundreds of tiles are walked by a whole wave (binning.hip:
    wave_for_each_tile); the lists must not change.  Mix of ordinary, large and screen-filling footprints,
    some anisotropic and rotated."""
    orc = oracle()
    d = cpu_stage_inputs(N, W, H, 0, 31)
    gen = torch.Generator().manual_seed(7)
    conic = d["conic"].clone()
    V = conic.shape[0]
    big = torch.rand(V, generator=gen) < 0.05
    grow = torch.where(torch.rand(V, generator=gen) < 0.3, 3e4, 4e2)   # sigma up to ~170 px
    conic[big] = conic[big] * grow[big].unsqueeze(1)
    huge = torch.nonzero(big)[:5, 0]
    conic[huge, 0] *= 50.0                                              # long thin ones across the screen
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    ref_s, ref_r = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], conic, ntx, nty, 3.0)
    counts = ref_r[1:] - ref_r[:-1]
    assert int(counts.min()) >= int(big.sum() * 0.2), "some Gaussians should cover every tile"
    got_s, got_r = hip_backend.get_sorted_gaussian_list(1024, d["uv"].to(DEV), d["xyz_c"].to(DEV), conic.to(DEV), ntx, nty,
                                                        3.0)
    assert torch.equal(got_r.cpu(), ref_r) and torch.equal(got_s.cpu(), ref_s)


def test_tile_lists_one_lane_per_gaussian(hip_backend):
    """more than 262144 visible Gaussians on a grid with too few of them per tile for the LDS histogram (binning.hip:
    for_subgroup_of, use_private): the atomic-counter kernels k_tile_count<1> / k_tile_emit<1>, one lane per Gaussian"""
    orc = oracle()
    W, H = 1920, 1080
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    d = cpu_stage_inputs(300000, W, H, 0, 14)
    V = d["uv"].shape[0]
    assert V > (1 << 18) and V * 8 <= 1024 * ntx * nty
    ref_sorted, ref_ranges = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], ntx, nty, 3.0)
    got_sorted, got_ranges = hip_backend.get_sorted_gaussian_list(
        1024, d["uv"].to(DEV), d["xyz_c"].to(DEV), d["conic"].to(DEV), ntx, nty, 3.0)
    assert torch.equal(got_ranges.cpu(), ref_ranges)
    assert torch.equal(got_sorted.cpu(), ref_sorted)
    assert ref_sorted.numel() > V


def _needs_tile_rows_extension(mod):
    if mod.__file__.endswith(".so"):
        pytest.skip("tile_rows= is an extension of the ctypes shim (multi-GPU hooks), not part of the "
                    "reference's signatures the native module mirrors")


def test_tile_lists_empty_and_row_restricted(hip_backend):
    _needs_tile_rows_extension(hip_backend)
    orc = oracle()
    e = torch.zeros(0, 2, device=DEV), torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV)
    s, r = hip_backend.get_sorted_gaussian_list(1024, e[0], e[1], e[2], 4, 3, 3.0)
    assert s.numel() == 0 and r.shape[0] == 13 and int(r.abs().sum()) == 0
    d = cpu_stage_inputs(8000, 320, 240, 0, 10)
    full_s, full_r = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], 20, 15, 3.0)
    got_s, got_r = hip_backend.get_sorted_gaussian_list(
        1024, d["uv"].to(DEV), d["xyz_c"].to(DEV), d["conic"].to(DEV), 20, 15, 3.0, tile_rows=(5, 9))
    got_s, got_r = got_s.cpu(), got_r.cpu()
    # owned tiles carry exactly the single-GPU lists, the others are empty
    for tile in range(20 * 15):
        n = int(got_r[tile + 1] - got_r[tile])
        if 5 * 20 <= tile < 9 * 20:
            a = full_s[full_r[tile]:full_r[tile + 1]]
            assert torch.equal(got_s[got_r[tile]:got_r[tile + 1]], a)
        else:
            assert n == 0


def test_tile_lists_band_of_a_grid_beyond_the_lds_histogram(hip_backend):
    """a grid of more than 16384 tiles (4 MP and up) whose band fits the LDS histogram and has enough Gaussians
    per tile for it (binning.hip: use_private decides on the BAND's tiles): the histogram matrix is PRIV_NB x band
    tiles and must fit the workspace gs_tile_workspace_ints sized from the grid.  Round-3 advisor finding: it did
    not, and the count pass wrote ~16 MB past the allocation.  Lists of the band == the oracle's, whole grid too."""
    _needs_tile_rows_extension(hip_backend)
    orc = oracle()
    W, H = 2320, 1840
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    assert ntx * nty > 16384
    rows = (60, 70)                      # 1450 tiles; LDS path needs V > 128 * 1450
    d = cpu_stage_inputs(260000, W, H, 0, 12)
    V = d["uv"].shape[0]
    assert V * 8 > 1024 * (rows[1] - rows[0]) * ntx
    full_s, full_r = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], ntx, nty, 3.0)
    dev = [d[k].to(DEV) for k in ("uv", "xyz_c", "conic")]
    guard = torch.full((1 << 22,), 7, dtype=torch.int32, device=DEV)   # a neighbour a stray write would land in
    got_s, got_r = hip_backend.get_sorted_gaussian_list(1024, *dev, ntx, nty, 3.0, tile_rows=rows)
    torch.cuda.synchronize()
    assert int((guard != 7).sum()) == 0
    got_s, got_r = got_s.cpu(), got_r.cpu()
    t0, t1 = rows[0] * ntx, rows[1] * ntx
    assert torch.equal(got_r[t0:t1 + 1] - got_r[t0], full_r[t0:t1 + 1] - full_r[t0])
    assert int(got_r[t0]) == 0 and int(got_r[-1]) == int(got_r[t1])
    assert torch.equal(got_s, full_s[full_r[t0]:full_r[t1]])
    # the whole grid (atomic-counter path: the grid itself is too large for the LDS histogram)
    all_s, all_r = hip_backend.get_sorted_gaussian_list(1024, *dev, ntx, nty, 3.0)
    assert torch.equal(all_r.cpu(), full_r) and torch.equal(all_s.cpu(), full_s)


# ---------------------------------------------------------------------------------------------------
# render forward: bit exact;  backward: 1e-4
# ---------------------------------------------------------------------------------------------------
def render_case(mod, dev, d, rgb, rays, bg, sorted_g, ranges, dtype, grad_image=None, tile_rows=None):
    c = lambda x: x.to(dev).to(dtype).contiguous() if x.is_floating_point() else x.to(dev).contiguous()
    H, W = d["H"], d["W"]
    img = torch.zeros(H, W, 3, dtype=dtype, device=dev)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=dev)
    fw = torch.zeros(H, W, dtype=dtype, device=dev)
    args = (c(d["uv"]), c(d["opacity"]), c(rgb), c(d["conic"]), c(rays), c(ranges), c(sorted_g), c(bg))
    kw = {} if tile_rows is None else dict(tile_rows=tile_rows)
    mod.render_tiles_cuda(*args, nsp, fw, img, **kw)
    out = dict(image=img.cpu(), nsp=nsp.cpu(), fw=fw.cpu())
    if grad_image is not None:
        grads = [torch.zeros_like(x) for x in (args[2], args[1], args[0], args[3])]
        mod.render_tiles_backward_cuda(*args, nsp, fw, c(grad_image), *grads, **kw)
        out.update(g_rgb=grads[0].cpu(), g_opacity=grads[1].cpu(), g_uv=grads[2].cpu(), g_conic=grads[3].cpu())
    return out


@pytest.mark.parametrize("N,W,H,seed,bgval", [(1000, 256, 256, 0, 0.0), (20000, 640, 472, 21, 0.5),
                                              (9000, 96, 80, 22, 0.5)])
def test_render_fp32_forward_bit_exact_and_backward(hip_backend, N, W, H, seed, bgval):
    """Config A, a mid-size scene with a partial last tile row (H=472), and a dense scene whose
    tiles hold > 960 splats (several LDS chunks on the GPU, and past the reference's first chunk:
    exercises the Q1 weight-update quirk)."""
    orc = oracle()
    d = cpu_stage_inputs(N, W, H, 0, seed)
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    sorted_g, ranges = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], ntx, nty, 3.0)
    rays = torch.zeros(1, 1, 1)
    bg = torch.full((3,), bgval)
    gi = make_grad_image(W, H, seed=seed + 1)
    ref = render_case(orc, "cpu", d, d["rgb"], rays, bg, sorted_g, ranges, torch.float32, gi)
    got = render_case(hip_backend, DEV, d, d["rgb"], rays, bg, sorted_g, ranges, torch.float32, gi)
    assert torch.equal(got["nsp"], ref["nsp"])
    assert torch.equal(got["fw"], ref["fw"])
    assert torch.equal(got["image"], ref["image"]), (got["image"] - ref["image"]).abs().max()
    if N == 9000:
        assert int((ranges[1:] - ranges[:-1]).max()) > 960
    for k in ("g_rgb", "g_opacity", "g_uv", "g_conic"):
        assert scaled_err(got[k], ref[k]) < 1e-5, f"{k}: {scaled_err(got[k], ref[k])}"
        assert rel_err(got[k], ref[k]) < GRAD_TOL, f"{k} elementwise: {rel_err(got[k], ref[k])}"


@pytest.mark.parametrize("n_sh", [4, 9, 16])
def test_render_per_pixel_sh_variants(hip_backend, n_sh):
    """render.cu:283-333 / render_backward.cu:422-488: per-pixel view-dependent colour"""
    orc = oracle()
    W, H = 160, 120
    d = cpu_stage_inputs(3000, W, H, 3, 30 + n_sh)
    sorted_g, ranges = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], 10, 8, 3.0)
    rays = compute_rays_in_world_frame(d["cam"], d["T"])
    coeffs = d["sh_coeffs"][:, :, :n_sh].contiguous()
    bg = torch.full((3,), 0.25)
    gi = make_grad_image(W, H, seed=77)
    ref = render_case(orc, "cpu", d, coeffs, rays, bg, sorted_g, ranges, torch.float32, gi)
    got = render_case(hip_backend, DEV, d, coeffs, rays, bg, sorted_g, ranges, torch.float32, gi)
    assert torch.equal(got["nsp"], ref["nsp"]) and torch.equal(got["image"], ref["image"])
    for k in ("g_rgb", "g_opacity", "g_uv", "g_conic"):
        assert scaled_err(got[k], ref[k]) < GRAD_TOL, f"{k}: {scaled_err(got[k], ref[k])}"


def test_render_per_pixel_sh_dense_lists(hip_backend):
    """The fp32 per-pixel-SH backward forms the colour-coefficient gradients in batches of 16 contributing splats
    per wave (a matrix-core contraction over the wave's 64 pixels): a scene with several chunks of 64 per tile and
    several full batches per wave and chunk, partial tiles on the right and bottom edges, every element checked."""
    orc = oracle()
    W, H = 200, 136   # 13 x 9 tiles, the last column / row partial
    d = cpu_stage_inputs(12000, W, H, 3, 91)
    sorted_g, ranges = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], 13, 9, 3.0)
    assert int((ranges[1:] - ranges[:-1]).max()) > 256
    rays = compute_rays_in_world_frame(d["cam"], d["T"])
    coeffs = d["sh_coeffs"].contiguous()
    bg = torch.full((3,), 0.1)
    gi = make_grad_image(W, H, seed=92)
    ref = render_case(orc, "cpu", d, coeffs, rays, bg, sorted_g, ranges, torch.float32, gi)
    got = render_case(hip_backend, DEV, d, coeffs, rays, bg, sorted_g, ranges, torch.float32, gi)
    assert torch.equal(got["nsp"], ref["nsp"]) and torch.equal(got["image"], ref["image"])
    for k in ("g_rgb", "g_opacity", "g_uv", "g_conic"):
        assert scaled_err(got[k], ref[k]) < 1e-5, f"{k}: {scaled_err(got[k], ref[k])}"
        assert rel_err(got[k], ref[k]) < GRAD_TOL, f"{k} elementwise: {rel_err(got[k], ref[k])}"
    # rows of Gaussians no pixel used stay exactly zero (nothing is added for an all-zero batch column)
    unused = torch.ones(coeffs.shape[0], dtype=torch.bool)
    unused[sorted_g.long()] = False
    assert not got["g_rgb"].cpu()[unused].any()


@pytest.mark.parametrize("N,W,H,deg,seed,rows", [(4000, 75, 53, 3, 201, None), (9000, 96, 80, 3, 202, None),
                                                 (2500, 333, 17, 2, 203, None), (7000, 160, 200, 1, 204, (3, 9)),
                                                 (300, 64, 64, 3, 205, None), (12000, 48, 48, 3, 206, None)])
def test_per_pixel_sh_backward_shapes(hip_backend, N, W, H, deg, seed, rows):
    """render_backward.cu:422-488 through the fp32 kernel (slots + MFMA batches) against the oracle on shapes that
    stress the batching: odd image sizes, a one-tile-row image, very long lists (48x48 with 12 k Gaussians: every wave
    fills many batches per chunk, hundreds of chunks), nearly empty tiles, a tile-row band.
    (The fp64 kernel on the device is no checker for it: the two precisions flip alpha >= 1/255 decisions against
    each other, each worth colour / 255 in the image.)"""
    orc = oracle()
    d = cpu_stage_inputs(N, W, H, deg, seed)
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    sorted_g, ranges = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], ntx, nty, 3.0)
    rays = compute_rays_in_world_frame(d["cam"], d["T"])
    coeffs = d["sh_coeffs"].contiguous()
    bg = torch.full((3,), 0.3)
    gi = make_grad_image(W, H, seed=seed + 1)
    if rows is not None:
        _needs_tile_rows_extension(hip_backend)
    kw = {} if rows is None else dict(tile_rows=rows)
    ref = render_case(orc, "cpu", d, coeffs, rays, bg, sorted_g, ranges, torch.float32, gi, **kw)
    got = render_case(hip_backend, DEV, d, coeffs, rays, bg, sorted_g, ranges, torch.float32, gi, **kw)
    assert torch.equal(got["nsp"], ref["nsp"]) and torch.equal(got["image"], ref["image"])
    for k in ("g_rgb", "g_opacity", "g_uv", "g_conic"):
        assert scaled_err(got[k], ref[k]) < 1e-5, f"{k}: {scaled_err(got[k], ref[k])}"
        assert rel_err(got[k], ref[k]) < GRAD_TOL, f"{k} elementwise: {rel_err(got[k], ref[k])}"
    assert got["g_rgb"].abs().max() > 0


@pytest.mark.parametrize("n_sh", [1, 16])
def test_render_fp64_parity(hip_backend, n_sh):
    orc = oracle()
    W, H = 96, 64
    d = cpu_stage_inputs(1500, W, H, 3, 40 + n_sh)
    sorted_g, ranges = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], 6, 4, 3.0)
    cam64 = Camera(W, H, d["cam"].K.double())
    rays = compute_rays_in_world_frame(cam64, d["T"].double())
    coeffs = d["rgb"] if n_sh == 1 else d["sh_coeffs"]
    bg = torch.full((3,), 0.5)
    gi = make_grad_image(W, H, seed=5)
    ref = render_case(orc, "cpu", d, coeffs, rays, bg, sorted_g, ranges, torch.float64, gi)
    got = render_case(hip_backend, DEV, d, coeffs, rays, bg, sorted_g, ranges, torch.float64, gi)
    assert torch.equal(got["nsp"], ref["nsp"])
    for k in ("image", "fw", "g_rgb", "g_opacity", "g_uv", "g_conic"):
        assert scaled_err(got[k], ref[k]) < 1e-11, f"{k}: {scaled_err(got[k], ref[k])}"


@pytest.mark.parametrize("mode", ["compat", "exact"])
@pytest.mark.parametrize("n_sh", [1, 16])
def test_render_fp64_backward_second_chunk(hip_backend, n_sh, mode):
    """The fp64 backward kernel stages its own chunks (256 splats with one colour coefficient, 64 with 16): one 16x16
    tile with 300 faint splats (the recipe of test_exact_backward_mode_is_the_derivative_of_the_forward), which every
    pixel composites to the end, so the kernel walks 2 resp. 5 chunks, the last one partial.  In compat mode the
    16-coefficient kernel's Q1 index (render_backward.cu:185) wraps at every 64th entry."""
    from gaussian_splatting_amd import _hip
    orc = oracle()
    gen = torch.Generator().manual_seed(7 + n_sh)
    V, W, H = 300, 16, 16
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    d = dict(W=W, H=H, uv=rnd(V, 2) * 16,
             conic=torch.stack([20 + 30 * rnd(V), 4 * (rnd(V) - 0.5), 20 + 30 * rnd(V)], dim=1),
             opacity=0.002 + 0.004 * rnd(V, 1))
    if n_sh == 1:
        coeffs, rays = rnd(V, 3), torch.zeros(1, 1, 1, dtype=torch.float64)
    else:
        coeffs = torch.cat((rnd(V, 3, 1), 0.2 * (rnd(V, 3, n_sh - 1) - 0.5)), dim=2)
        rays = torch.randn(H, W, 3, generator=gen, dtype=torch.float64)
        rays = rays / rays.norm(dim=2, keepdim=True)
    bg = torch.full((3,), 0.3, dtype=torch.float64)
    gi = torch.randn(H, W, 3, generator=gen, dtype=torch.float64)
    ranges = torch.tensor([0, V], dtype=torch.int32)
    sorted_g = torch.arange(V, dtype=torch.int32)
    try:
        _hip.set_backward_mode(mode)
        orc.set_backward_exact(int(mode == "exact"))
        ref = render_case(orc, "cpu", d, coeffs, rays, bg, sorted_g, ranges, torch.float64, gi)
        got = render_case(hip_backend, DEV, d, coeffs, rays, bg, sorted_g, ranges, torch.float64, gi)
    finally:
        _hip.set_backward_mode("compat")
        orc.set_backward_exact(0)
    assert int(ref["nsp"].min()) == V   # nobody saturates: every pixel walks all 300 splats
    assert torch.equal(got["nsp"], ref["nsp"])
    for k in ("image", "fw", "g_rgb", "g_opacity", "g_uv", "g_conic"):
        assert scaled_err(got[k], ref[k]) < 1e-11, f"{k}: {scaled_err(got[k], ref[k])}"


def test_render_tile_row_restriction(hip_backend):
    _needs_tile_rows_extension(hip_backend)
    orc = oracle()
    W, H = 320, 240
    d = cpu_stage_inputs(8000, W, H, 0, 50)
    sorted_g, ranges = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], 20, 15, 3.0)
    bg = torch.full((3,), 0.5)
    gi = make_grad_image(W, H, seed=6)
    full = render_case(hip_backend, DEV, d, d["rgb"], torch.zeros(1, 1, 1), bg, sorted_g, ranges, torch.float32, gi)
    parts = [render_case(hip_backend, DEV, d, d["rgb"], torch.zeros(1, 1, 1), bg, sorted_g, ranges, torch.float32,
                         gi, tile_rows=r) for r in ((0, 4), (4, 11), (11, 15))]
    img = sum(p["image"] for p in parts)
    assert torch.equal(img, full["image"])      # untouched rows stay zero: the bands tile the image
    for k in ("g_rgb", "g_opacity", "g_uv", "g_conic"):
        s = sum(p[k] for p in parts)
        assert scaled_err(s, full[k]) < 1e-5, k


def test_depth_parity(hip_backend):
    orc = oracle()
    W, H = 320, 240
    d = cpu_stage_inputs(8000, W, H, 0, 60)
    sorted_g, ranges = orc.get_sorted_gaussian_list(1024, d["uv"], d["xyz_c"], d["conic"], 20, 15, 3.0)
    ref = torch.full((H, W, 1), -1.0)
    orc.render_depth_cuda(d["xyz_c"], d["uv"], d["opacity"], d["conic"], ranges, sorted_g, 0.2, ref)
    got = torch.full((H, W, 1), -1.0, device=DEV)
    hip_backend.render_depth_cuda(d["xyz_c"].to(DEV), d["uv"].to(DEV), d["opacity"].to(DEV), d["conic"].to(DEV),
                                  ranges.to(DEV), sorted_g.to(DEV), 0.2, got)
    assert torch.equal(got.cpu(), ref)
    assert (ref > 0).float().mean() > 0.5


# ---------------------------------------------------------------------------------------------------
# end to end through the host mirror
# ---------------------------------------------------------------------------------------------------
def test_rasterize_reference_known_answers_on_gpu(hip_backend):
    """test/test_rasterize.py:21-54 and test/test_depth.py:17-36 on the HIP path"""
    g, cam, T, fx = scene6(DEV)
    img, mask, uv = rasterize(g, T, cam, 0.3, 100.0, 10, 3.0, True, torch.zeros(3, device=DEV))
    for ch, v in enumerate([0.47698545455932617, 0.0, 0.0]):
        assert abs(img[340, 348, ch].item() - v) < 5e-6
    for ch, v in enumerate([0.03330837935209274, 0.0, 0.267561137676239]):
        assert abs(img[200, 348, ch].item() - v) < 5e-6
    ys, xs = fx["sub_ys"], fx["sub_xs"]
    assert np.abs(img.cpu().numpy()[np.ix_(ys, xs)] - fx["nosh_image_sub"]).max() < 1e-5
    d = render_depth(g, 0.2, T, cam, 0.3, 10, 3.0)
    assert abs(d[340, 348].item() - 17.29551887512207) < 5e-6
    assert abs(d[200, 348].item() - 13.205718040466309) < 5e-6
    # SH through the shipped header (what the CUDA path computes)
    g.sh = torch.ones((6, 3, 15), device=DEV) * 0.1
    for mode, pre in (("sh_pre", True), ("sh_pix", False)):
        img, _, _ = rasterize(g, T, cam, 0.3, 100.0, 10, 3.0, pre, torch.zeros(3, device=DEV))
        assert np.abs(img.cpu().numpy()[np.ix_(ys, xs)] - fx[f"{mode}_image_sub"]).max() < 1e-5


@pytest.mark.parametrize("tag", ["deg0", "deg3_pre", "deg3_pix"])
def test_rasterize_matches_reference_host_fixtures(hip_backend, tag):
    """full pipeline, forward + backward to dense parameter gradients, against what the reference
    host produced over the oracle.  The PyTorch glue (matmul, sigmoid, inverse) runs on the GPU here
    and on the CPU there, so inputs of the kernels differ in the last ulp: tolerance, not equality."""
    fx = load(f"ref_host_synth_{tag}.npz")
    g, cam, T = scene_from_fixture(fx, DEV, requires_grad=True)
    img, mask, uv = rasterize(g, T, cam, float(fx["near"]), float(fx["far"]), int(fx["padding"]),
                              float(fx["mh_dist"]), bool(fx["use_sh_precompute"]), t(fx["background"], DEV))
    uv.retain_grad()
    (img * t(fx["grad_image"], DEV)).sum().backward()
    assert np.array_equal(mask.cpu().numpy(), fx["mask"])
    assert np.abs(uv.detach().cpu().numpy() - fx["uv"]).max() < 1e-3
    # a one-ulp input difference can flip an alpha >= 1/255 decision: bound the image by 1e-5 on
    # all but a handful of pixels and by the largest single-splat contribution everywhere
    diff = np.abs(img.detach().cpu().numpy() - fx["image"]).max(axis=2)
    assert (diff > 1e-5).mean() < 2e-3 and diff.max() < 5e-3, (float((diff > 1e-5).mean()), float(diff.max()))
    assert scaled_err(uv.grad, t(fx["grad_uv"])) < 5e-3
    for k in ("xyz", "rgb", "opacity", "scale", "quaternion", "sh"):
        if "grad_" + k in fx.files:
            e = scaled_err(getattr(g, k).grad, t(fx["grad_" + k]))
            assert e < 5e-3, f"{k}: {e}"


def test_uv_retain_grad_semantics(hip_backend):
    """trainer.py:360,379: the returned uv is the post-cull intermediate and its .grad is grad_uv"""
    g, cam, T = make_scene(500, 128, 96, 0, seed=70, device=DEV)
    for p in (g.xyz, g.rgb, g.opacity, g.scale, g.quaternion):
        p.requires_grad_(True)
    img, mask, uv = rasterize(g, T, cam, 0.3, 500.0, 100, 3.0, True, torch.zeros(3, device=DEV))
    uv.retain_grad()
    img.sum().backward()
    assert uv.grad is not None and uv.grad.shape == uv.shape == (int((~mask).sum()), 2)
    assert g.xyz.grad.shape == g.xyz.shape and torch.isfinite(g.xyz.grad).all()
    assert (g.xyz.grad[mask] == 0).all()


# ---------------------------------------------------------------------------------------------------
# the reference's own fp64 gradcheck recipes on the HIP path
# ---------------------------------------------------------------------------------------------------
def test_gradcheck_per_gaussian_hip(hip_backend):
    from .test_oracle_gradcheck import run_per_gaussian_gradchecks
    run_per_gaussian_gradchecks(DEV)


@pytest.mark.parametrize("n_sh", [1, 4, 9, 16])
def test_gradcheck_sh_hip(hip_backend, n_sh):
    from .test_oracle_gradcheck import run_sh_gradcheck
    run_sh_gradcheck(n_sh, DEV)


@pytest.mark.parametrize("n_sh", [1, 4, 9, 16])
@pytest.mark.parametrize("bgval", [0.5, 0.0])
def test_gradcheck_render_hip(hip_backend, n_sh, bgval):
    from .test_oracle_gradcheck import run_render_gradcheck
    run_render_gradcheck(n_sh, bgval, DEV)


# ---------------------------------------------------------------------------------------------------
# error behaviour at the boundary (src/checks.cuh, render.cu:204-246,334-335)
# ---------------------------------------------------------------------------------------------------
def test_error_behaviour(hip_backend):
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
    with pytest.raises(RuntimeError, match="contiguous"):
        hip_backend.camera_projection_cuda(z(4, 6)[:, ::2], z(3, 3), z(4, 2))
    with pytest.raises(RuntimeError, match="float32 or float64"):
        hip_backend.camera_projection_cuda(z(4, 3, dtype=torch.float16), z(3, 3), z(4, 2))
    with pytest.raises(RuntimeError, match="double"):
        hip_backend.camera_projection_cuda(z(4, 3, dtype=torch.float64), z(3, 3), z(4, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="SH"):
        hip_backend.precompute_rgb_from_sh_cuda(z(4, 3), z(4, 3, 5), z(4, 4), z(4, 3))
    with pytest.raises(RuntimeError, match="Nx1"):
        hip_backend.render_tiles_cuda(z(4, 2), z(4), z(4, 3), z(4, 3), z(1, 1, 1), z(5, dtype=torch.int32),
                                      z(0, dtype=torch.int32), z(3), z(32, 32, dtype=torch.int32), z(32, 32),
                                      z(32, 32, 3))
    with pytest.raises(RuntimeError, match="int tensor"):
        hip_backend.render_tiles_cuda(z(4, 2), z(4, 1), z(4, 3), z(4, 3), z(1, 1, 1), z(5, dtype=torch.int64),
                                      z(0, dtype=torch.int32), z(3), z(32, 32, dtype=torch.int32), z(32, 32),
                                      z(32, 32, 3))


# ---------------------------------------------------------------------------------------------------
# gradient mode: compat (render_backward.cu:185) vs exact
# ---------------------------------------------------------------------------------------------------
def test_exact_backward_mode_is_the_derivative_of_the_forward():
    """fp64 (no alpha threshold: the forward is smooth), 400 faint splats on one tile, so every pixel
    composites past the reference's first fp64 chunk (320).  A central difference of the forward along a
    random direction equals <gradient, direction> in GS_BACKWARD_EXACT mode and does not in the default
    compat mode (the weights beyond the first chunk carry the factor 1 / (1 - alpha_last)); the oracle's
    exact mode agrees with the kernel's."""
    from gaussian_splatting_amd import _hip, splat_cuda
    from oracle import gs_oracle as orc
    gen = torch.Generator().manual_seed(3)
    V, W, H = 400, 16, 16
    uv = (torch.rand(V, 2, generator=gen, dtype=torch.float64) * 16)
    conic = torch.stack([20 + 30 * torch.rand(V, generator=gen, dtype=torch.float64),
                         4 * (torch.rand(V, generator=gen, dtype=torch.float64) - 0.5),
                         20 + 30 * torch.rand(V, generator=gen, dtype=torch.float64)], dim=1)
    opacity = 0.002 + 0.004 * torch.rand(V, 1, generator=gen, dtype=torch.float64)
    rgb = torch.rand(V, 3, generator=gen, dtype=torch.float64)
    bg = torch.full((3,), 0.3, dtype=torch.float64)
    gi = torch.randn(H, W, 3, generator=gen, dtype=torch.float64)
    ranges = torch.tensor([0, V], dtype=torch.int32)
    sorted_g = torch.arange(V, dtype=torch.int32)
    rays = torch.zeros(1, 1, 1, dtype=torch.float64)
    inputs = [uv, opacity, rgb, conic]
    direction = [torch.randn(t.shape, generator=gen, dtype=torch.float64) * s
                 for t, s in zip(inputs, (1e-2, 1e-4, 1e-2, 1e-1))]

    def forward(mod, dev, ts):
        img = torch.zeros(H, W, 3, dtype=torch.float64, device=dev)
        nsp = torch.zeros(H, W, dtype=torch.int32, device=dev)
        fw = torch.zeros(H, W, dtype=torch.float64, device=dev)
        a = [t.to(dev).contiguous() for t in ts]
        mod.render_tiles_cuda(a[0], a[1], a[2], a[3], rays.to(dev), ranges.to(dev), sorted_g.to(dev), bg.to(dev), nsp, fw, img)
        return img, nsp, fw, a

    def backward(mod, dev, ts):
        img, nsp, fw, a = forward(mod, dev, ts)
        g = [torch.zeros(V, 3, dtype=torch.float64, device=dev), torch.zeros(V, 1, dtype=torch.float64, device=dev),
             torch.zeros(V, 2, dtype=torch.float64, device=dev), torch.zeros(V, 3, dtype=torch.float64, device=dev)]
        mod.render_tiles_backward_cuda(a[0], a[1], a[2], a[3], rays.to(dev), ranges.to(dev), sorted_g.to(dev), bg.to(dev),
                                       nsp, fw, gi.to(dev), *g)
        assert int(nsp.min()) == V   # nobody saturates: every pixel walks all 400 splats
        return {"uv": g[2].cpu(), "opacity": g[1].cpu(), "rgb": g[0].cpu(), "conic": g[3].cpu()}

    h = 1e-4
    plus = forward(splat_cuda, DEV, [t + h * d for t, d in zip(inputs, direction)])[0].cpu()
    minus = forward(splat_cuda, DEV, [t - h * d for t, d in zip(inputs, direction)])[0].cpu()
    numeric = float(((plus - minus) / (2 * h) * gi).sum())

    def directional(grads):
        return float(sum((grads[k] * d).sum() for k, d in zip(("uv", "opacity", "rgb", "conic"), direction)))

    try:
        _hip.set_backward_mode("exact")
        orc.set_backward_exact(1)
        exact = backward(splat_cuda, DEV, inputs)
        ref_exact = backward(orc, "cpu", inputs)
    finally:
        _hip.set_backward_mode("compat")
        orc.set_backward_exact(0)
    compat = backward(splat_cuda, DEV, inputs)
    ref_compat = backward(orc, "cpu", inputs)
    assert abs(directional(exact) - numeric) < 1e-6 * abs(numeric), (directional(exact), numeric)
    assert abs(directional(compat) - numeric) > 1e-4 * abs(numeric), "Q1 should be visible past the first chunk"
    for k in exact:
        assert scaled_err(exact[k], ref_exact[k]) < 1e-11, k
        assert scaled_err(compat[k], ref_compat[k]) < 1e-11, k
