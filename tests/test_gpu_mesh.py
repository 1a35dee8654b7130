"""The TSDF fusion and mesh extraction kernels (csrc/tsdf.hip, ABI 24) and gaussian_splatting_amd/mesh.py on the GPU
against the float64 restatement of their definitions (tests/mesh_ref.py, checked on its own by tests/test_mesh_ref.py):

  integration   tsdf, weight and color with ref64.r_measure, env = |restatement in fp32 - restatement in fp64|, bound
                R_MAX = 8 (tests/test_gpu_general_cameras.py), on the nodes the left-out rule keeps (at most LEFT_OUT_CAP of
                them left out, asserted); weight exactly equal there.  Untouched nodes keep the bits of a NaN-bearing
                pattern; a batch of C views gives the bits of C calls; image / color NULL together or GS_EINVAL.
  extraction    on volumes the test writes, so that every sign decision is exact: faces equal to the reference's after
                rotating each to its smallest index first and sorting, vertices and colours by r_measure, two calls
                bit-equal, and on the sphere the closed-manifold and orientation properties on the kernel's own mesh.
  plumbing      mesh.integrate_frame equals render, mask, integrate done by hand, bit for bit."""
import functools
import types

import numpy as np
import pytest
import torch

from gaussian_splatting_amd import _hip, fused, mesh
from gaussian_splatting_amd.synthetic import make_scene

from . import mesh_ref as R
from .helpers import report
from .ref64 import r_measure

pytestmark = pytest.mark.gpu

R_MAX = 8.0   # tests/test_gpu_general_cameras.py
DEV = "cuda:0"


def dev(a, dtype=torch.float32):
    """a device tensor of its own: the shared cases are never written through it"""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).clone().to(DEV)


def volume_of(dims, origin, voxel, state=None, with_color=True, **kw):
    vol = mesh.TSDFVolume(origin, voxel, dims, with_color=with_color, device=DEV, **kw)
    if state is not None:
        vol.tsdf, vol.weight = dev(state[0]), dev(state[1])
        vol.color = dev(state[2]) if with_color else None
    return vol


def case_volume(case, **kw):
    return volume_of(case["dims"], case["origin"], R.VOXEL, case["start"], sdf_trunc=R.SDF_TRUNC, max_weight=R.MAX_WEIGHT, **kw)


def integrate_case(vol, case, fisheye, views=slice(None), with_image=True):
    vol.integrate_views(dev(case["depth"][views]), dev(case["cams"][views]), dev(case["Ks"][views]),
                        dev(case["image"][views]) if with_image else None,
                        camera_model="fisheye" if fisheye else "pinhole", near_thresh=R.NEAR, depth_max=R.DEPTH_MAX)
    return vol


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1: integration against the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("fisheye", (False, True), ids=("pinhole", "fisheye"))
@pytest.mark.parametrize("volume", tuple(R.VOLUMES))
def test_integration_against_the_reference(volume, fisheye):
    case = R.integration_case(volume, fisheye)
    vol = integrate_case(case_volume(case), case, fisheye)
    keep = ~case["left_out"]
    vals = dict(left_out=float(case["left_out"].mean()))
    got = dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), color=vol.color.cpu().numpy())
    for a, name in enumerate(("tsdf", "weight", "color")):
        f64, f32 = case["f64"][a][keep], case["f32"][a][keep].astype(np.float64)
        col = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).reshape(-1, 1)
        vals["r_" + name] = r_measure(col(got[name][keep]), col(f64), col(f32 - f64))
    updated = case["f64"][1] != case["start"][1]
    vals["updated"] = float(updated.mean())
    report(f"tsdf_integrate[{volume}, {'fisheye' if fisheye else 'pinhole'}]", **vals)
    print(vals)
    assert vals["left_out"] <= R.LEFT_OUT_CAP
    assert vals["r_tsdf"] <= R_MAX and vals["r_color"] <= R_MAX, vals
    assert np.array_equal(got["weight"][keep], case["f64"][1][keep].astype(np.float32))
    # kept nodes that the reference leaves alone keep their bits
    alone = keep & ~updated
    for a, name in enumerate(("tsdf", "weight", "color")):
        assert np.array_equal(got[name][alone], case["start"][a][alone]), name


@pytest.mark.parametrize("fisheye", (False, True), ids=("pinhole", "fisheye"))
def test_extraction_of_the_fused_volume_equals_the_reference(fisheye):
    """test 6: the volume fused in test 1, extracted by the kernels and by the reference from the same device tensors"""
    case = R.integration_case("24x20x16", fisheye)
    vol = integrate_case(case_volume(case), case, fisheye)
    check_extraction(vol, f"fused[{'fisheye' if fisheye else 'pinhole'}]", min_faces=100)


# ---- 2: untouched nodes keep their bits ----------------------------------------------------------------------------------
def pattern_state(dims, seed=9):
    """weights 0..3; NaN in tsdf and color where the weight is 0"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    weight = rng.integers(0, 4, (nz, ny, nx)).astype(np.float32)
    tsdf = np.where(weight > 0, rng.uniform(-1, 1, (nz, ny, nx)), np.nan).astype(np.float32)
    color = np.where(weight[..., None] > 0, rng.uniform(0, 1, (nz, ny, nx, 3)), np.nan).astype(np.float32)
    return tsdf, weight, color


@pytest.mark.parametrize("fisheye", (False, True), ids=("pinhole", "fisheye"))
def test_untouched_nodes_keep_their_bits(fisheye):
    case = R.integration_case("24x20x16", fisheye)
    start = pattern_state(case["dims"])
    vol = volume_of(case["dims"], case["origin"], R.VOXEL, start, sdf_trunc=R.SDF_TRUNC)
    before = [bits(t).clone() for t in (vol.tsdf, vol.weight, vol.color)]
    integrate_case(vol, case, fisheye)
    # what the float64 reference updates from the same start (NaN state stays NaN there too, but its weight moves)
    ref = R.integrate_ref(start, case["depth"], case["image"], case["cams"], case["Ks"], fisheye, R.NEAR, R.SDF_TRUNC, 64.0,
                          R.DEPTH_MAX, case["origin"], R.VOXEL, case["dims"], np.float64)
    untouched = torch.from_numpy((ref[1] == start[1]) & ~case["left_out"]).to(DEV)
    assert 0.2 < float(untouched.float().mean()) < 0.8
    for b, t in zip(before, (vol.tsdf, vol.weight, vol.color)):
        assert torch.equal(bits(t)[untouched], b[untouched])
    touched = torch.from_numpy((ref[1] != start[1]) & ~case["left_out"]).to(DEV)
    assert torch.equal(vol.weight[touched], dev(ref[1])[touched])
    # views that see nothing change nothing: behind the camera, looking away, all pixels invalid, beyond the truncation
    after = [bits(t).clone() for t in (vol.tsdf, vol.weight, vol.color)]
    M = case["cams"].copy()
    behind = M.copy()
    behind[0, 2, 3] = -3.0                      # the volume at z < 0
    away = M.copy()
    away[0, 0, 3] = 50.0                        # far outside the image
    model = "fisheye" if fisheye else "pinhole"
    for cams, depth in ((behind, case["depth"]), (away, case["depth"]), (M, np.zeros_like(case["depth"])),
                        (M, np.full_like(case["depth"], np.nan)), (M, np.full_like(case["depth"], 0.25)),
                        (M, np.full_like(case["depth"], R.DEPTH_MAX * 2))):
        vol.integrate_views(dev(depth), dev(cams), dev(case["Ks"]), dev(case["image"]), camera_model=model, near_thresh=R.NEAR,
                            depth_max=R.DEPTH_MAX)
        for b, t in zip(after, (vol.tsdf, vol.weight, vol.color)):
            assert torch.equal(bits(t), b)


# ---- 3: a batch equals single calls --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_views(C, fisheye):
    """C views around the yawed one of test 1, each with its own depth map and image"""
    cams, Ks, depths, images = [], [], [], []
    for c in range(C):
        M, K = R.view_camera(yaw=0.3 - 0.07 * c, shift=(0.02 * c, -0.01 * c, 0.03 * (c % 3)))
        d, im = R.view_depth(M, K, fisheye, radius=0.3 + 0.01 * c)
        cams.append(M), Ks.append(K), depths.append(d), images.append(np.roll(im, c, axis=1))
    return dict(cams=np.stack(cams), Ks=np.stack(Ks), depth=np.stack(depths), image=np.stack(images))


@pytest.mark.parametrize("fisheye", (False, True), ids=("pinhole", "fisheye"))
@pytest.mark.parametrize("C", (1, 3, 9))   # the kernel stages no cameras: there is no chunk size to step over
def test_a_batch_equals_single_view_calls(C, fisheye):
    dims = R.VOLUMES["65x9x5"] if C == 3 else R.VOLUMES["24x20x16"]
    views = batch_views(C, fisheye)
    make = lambda: volume_of(dims, R.volume_origin(dims), R.VOXEL, R.start_state(dims), sdf_trunc=R.SDF_TRUNC)
    batch = integrate_case(make(), views, fisheye)
    single = make()
    for c in range(C):
        integrate_case(single, views, fisheye, views=slice(c, c + 1))
    for a, b in ((batch.tsdf, single.tsdf), (batch.weight, single.weight), (batch.color, single.color)):
        assert torch.equal(bits(a), bits(b))
    assert bool(torch.isfinite(batch.tsdf).all())
    assert float((batch.weight - dev(R.start_state(dims)[1])).max()) == C   # some node is updated by every view
    # and through integrate(), the one-view entry of the interface
    if C == 3:
        one = make()
        for c in range(C):
            one.integrate(dev(views["depth"][c]), dev(views["cams"][c]), types.SimpleNamespace(K=dev(views["Ks"][c])),
                          dev(views["image"][c]), camera_model="fisheye" if fisheye else "pinhole", near_thresh=R.NEAR,
                          depth_max=R.DEPTH_MAX)
        assert torch.equal(bits(one.tsdf), bits(batch.tsdf)) and torch.equal(bits(one.color), bits(batch.color))


def test_the_weight_stops_at_max_weight():
    case = R.integration_case("24x20x16", False)
    rep = lambda a: np.repeat(a, 70, axis=0)
    views = dict(depth=rep(case["depth"]), cams=rep(case["cams"]), Ks=rep(case["Ks"]), image=rep(case["image"]))
    vol = volume_of(case["dims"], case["origin"], R.VOXEL, sdf_trunc=R.SDF_TRUNC, max_weight=64.0)
    integrate_case(vol, views, False)
    seen = vol.weight > 0
    assert 0.3 < float(seen.float().mean()) < 0.95
    assert bool((vol.weight[seen] == 64.0).all()) and bool(torch.isfinite(vol.tsdf).all()) and bool(torch.isfinite(vol.color).all())
    assert bool((vol.tsdf[~seen] == 1).all()) and not vol.color[~seen].any()
    # the same view over and over: the average of equal values |t| <= 1 stays within rounding of the value -- three
    # roundings of at most 2^-24 (relative to a result of at most 1) in each of the 70 steps
    once = integrate_case(volume_of(case["dims"], case["origin"], R.VOXEL, sdf_trunc=R.SDF_TRUNC), case, False)
    assert float((vol.tsdf - once.tsdf).abs().max()) <= 70 * 3 * 2.0 ** -24


# ---- 4: colour is optional, but image and color go together ---------------------------------------------------------------
def test_without_colour_and_exactly_one_of_image_and_color():
    case = R.integration_case("24x20x16", False)
    grey = integrate_case(case_volume(case, with_color=False), case, False, with_image=False)
    full = integrate_case(case_volume(case), case, False)
    assert grey.color is None
    assert torch.equal(bits(grey.tsdf), bits(full.tsdf)) and torch.equal(bits(grey.weight), bits(full.weight))
    v, f, c = grey.extract_mesh()
    assert c is None and len(v) > 0 and len(f) > 0
    # at the C ABI: exactly one of the two is GS_EINVAL and writes nothing
    vol = case_volume(case)
    before = [t.clone() for t in (vol.tsdf, vol.weight, vol.color)]
    p = _hip.ptr
    d, im, M, K = (dev(case[k]) for k in ("depth", "image", "cams", "Ks"))
    W, H = R.FRAME
    tail = (1, W, H, _hip.GS_RASTER_CLASSIC, R.NEAR, R.SDF_TRUNC, 64.0, R.DEPTH_MAX, *vol.origin, vol.voxel_size, *vol.dims)
    lib = _hip.lib()
    assert lib.gs_tsdf_integrate(p(d), None, p(M), p(K), *tail, p(vol.tsdf), p(vol.weight), p(vol.color), None) == _hip.GS_EINVAL
    assert lib.gs_tsdf_integrate(p(d), p(im), p(M), p(K), *tail, p(vol.tsdf), p(vol.weight), None, None) == _hip.GS_EINVAL
    torch.cuda.synchronize()
    for b, t in zip(before, (vol.tsdf, vol.weight, vol.color)):
        assert torch.equal(bits(t), bits(b))


# ---- 5: extraction --------------------------------------------------------------------------------------------------------
def check_extraction(vol, tag, level=0.0, min_weight=1.0, min_faces=0):
    """extract_mesh against the reference's extraction of the same device tensors -> the kernel's mesh as numpy arrays"""
    v, f, c = vol.extract_mesh(level, min_weight)
    v2, f2, c2 = vol.extract_mesh(level, min_weight)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    assert torch.equal(bits(v), bits(v2)) and torch.equal(f, f2)
    state = (vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), None if vol.color is None else vol.color.cpu().numpy())
    ref = {dt: R.extract_ref(*state, vol.origin, vol.voxel_size, level, min_weight, dt) for dt in (np.float64, np.float32)}
    r64, r32 = ref[np.float64], ref[np.float32]
    assert len(r64["faces"]) >= min_faces
    assert v.shape[0] == len(r64["vertices"]) and f.shape[0] == len(r64["faces"])
    fa = f.cpu().numpy()
    assert np.array_equal(R.canonical_faces(fa), R.canonical_faces(r64["faces"]))
    # ordered by (cell, q, triangle): face by face the same triangle, whichever corner comes first
    assert np.array_equal(np.sort(fa, 1), np.sort(r64["faces"], 1))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    vals = dict(vertices=len(r64["vertices"]), faces=len(r64["faces"]),
                r_vertices=r_measure(v, t(r64["vertices"]), t(r32["vertices"]) - t(r64["vertices"])))
    if vol.color is None:
        assert c is None and c2 is None
    else:
        assert torch.equal(bits(c), bits(c2)) and c.shape == v.shape
        vals["r_colors"] = r_measure(c, t(r64["colors"]), t(r32["colors"]) - t(r64["colors"]))
    report(f"tsdf_extract[{tag}]", **vals)
    print(tag, vals)
    assert vals["r_vertices"] <= R_MAX and vals.get("r_colors", 0.0) <= R_MAX, vals
    return v.cpu().numpy(), fa, r64


def test_extraction_of_the_sphere():
    tsdf, weight, color = R.sphere_volume()
    nx, ny, nz = R.SPHERE["dims"]
    vol = volume_of((nx, ny, nz), (0, 0, 0), 1.0, (tsdf, weight, color))
    v, f, ref = check_extraction(vol, "sphere")
    assert (len(v), len(f)) == (1228, 2452)
    # the properties of tests/test_mesh_ref.py on the kernel's own mesh
    assert R.is_closed_manifold(f) and R.euler_characteristic(len(v), f) == 2
    nrm, cen = R.face_normals_and_centroids(v, f)
    assert (np.linalg.norm(nrm, axis=1) > 0).all()
    assert ((nrm * (cen - np.asarray(R.SPHERE["centre"]))).sum(1) > 0).all()
    err = np.abs(np.linalg.norm(v.astype(np.float64) - np.asarray(R.SPHERE["centre"]), axis=1) - R.SPHERE["radius"])
    assert err.max() <= R.sphere_radial_bound()
    # an origin and a voxel size that are not 0 and 1, a level that is not 0, no colour
    vol = volume_of((nx, ny, nz), (0.37, -1.2, 2.5), 0.013, (tsdf, weight, None), with_color=False)
    check_extraction(vol, "sphere, level 0.4", level=0.4)


def test_extraction_of_a_random_volume_with_holes():
    tsdf, weight, color = R.random_volume()
    nz, ny, nx = tsdf.shape
    vol = volume_of((nx, ny, nz), (-0.3, 0.1, 0.7), 0.25, (tsdf, weight, color))
    _, f, ref = check_extraction(vol, "random 9x7x6", min_faces=200)
    # the volume is worth its place: every sign case in all six tetrahedra, inactive cells next to active ones
    assert ref["tet_cases"] == {(q, c) for q in range(6) for c in range(16)}
    act = ref["active"]
    assert act.any() and not act.all() and (act[:, :, 1:] != act[:, :, :-1]).any()
    # min_weight decides what is observed: weights are 0 or 2 here
    v3, f3, _ = vol.extract_mesh(min_weight=3.0)
    assert v3.shape == (0, 3) and f3.shape == (0, 3)
    # weight holes with NaN behind them, as a fused volume has them nowhere but could
    tsdf2 = np.where(weight > 0, tsdf, np.nan).astype(np.float32)
    vol2 = volume_of((nx, ny, nz), (-0.3, 0.1, 0.7), 0.25, (tsdf2, weight, color))
    _, f2, _ = check_extraction(vol2, "random 9x7x6, NaN in the holes", min_faces=200)
    assert np.array_equal(f2, f)


@pytest.mark.parametrize("name", ("no crossing", "nx = 1", "ny = 1", "nz = 1", "nothing observed"))
def test_extraction_that_finds_nothing(name):
    tsdf, weight, color = R.random_volume()
    if name == "no crossing":
        tsdf = np.abs(tsdf) + 0.1
    elif name == "nothing observed":
        weight = np.zeros_like(weight)
    else:
        sl = {"nx = 1": np.s_[:, :, :1], "ny = 1": np.s_[:, :1, :], "nz = 1": np.s_[:1, :, :]}[name]
        tsdf, weight, color = (np.ascontiguousarray(a[sl]) for a in (tsdf, weight, color))
    nz, ny, nx = tsdf.shape
    vol = volume_of((nx, ny, nz), (0, 0, 0), 1.0, (tsdf, weight, color))
    v, f, c = vol.extract_mesh()
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.device == vol.tsdf.device
    ref = R.extract_ref(tsdf, weight, color, (0, 0, 0), 1.0, 0.0, 1.0, np.float64)
    assert len(ref["vertices"]) == 0 and len(ref["faces"]) == 0


@pytest.mark.parametrize("inside", (0b00000001, 0b10000000, 0b01101001, 0b11110000, 0b01111111, 0b10110010))
def test_extraction_of_a_single_cell(inside):
    rng = np.random.default_rng(inside)
    mag = rng.uniform(0.1, 1.0, 8)
    sign = np.array([-1.0 if inside >> c & 1 else 1.0 for c in range(8)])
    tsdf = (mag * sign).reshape(2, 2, 2).astype(np.float32)
    color = rng.uniform(0, 1, (2, 2, 2, 3)).astype(np.float32)
    vol = volume_of((2, 2, 2), (1.0, 2.0, 3.0), 0.5, (tsdf, np.ones_like(tsdf), color))
    v, f, _ = check_extraction(vol, f"one cell {inside:08b}", min_faces=1)
    assert R.interior_edges_are_paired(f)
    # every face looks from the inside corners towards the outside ones
    nrm, cen = R.face_normals_and_centroids(v, f)
    corners = np.array([[c & 1, c >> 1 & 1, c >> 2] for c in range(8)], dtype=np.float64) * 0.5 + np.array([1.0, 2.0, 3.0])
    ins = np.array([bool(inside >> c & 1) for c in range(8)])
    if ins.sum() in (1, 7):   # one corner cut off: its normal points away from (towards) that corner
        lone = corners[ins][0] if ins.sum() == 1 else corners[~ins][0]
        s = ((cen - lone) * nrm).sum(1)
        assert (s > 0).all() if ins.sum() == 1 else (s < 0).all()


# ---- 7: integrate_frame is render, mask, integrate -------------------------------------------------------------------------
@pytest.mark.parametrize("depth", ("median", "expected"))
def test_integrate_frame_is_render_mask_integrate(depth):
    W, H = R.FRAME
    g, cam, T = make_scene(300, W, H, 0, seed=4, device=DEV)
    g.opacity.add_(2.0)
    bg = torch.full((3,), 0.25, device=DEV)
    args = dict(near_thresh=0.3, far_thresh=500.0, cull_mask_padding=100, mh_dist=3.0)
    make = lambda: mesh.TSDFVolume((-2.0, -1.5, 1.4), 0.12, (33, 25, 40), device=DEV)
    vol = make()
    image, fused_depth = mesh.integrate_frame(vol, g, T, cam, background_rgb=bg, depth=depth, min_alpha=0.5, **args)
    by_hand = make()
    with torch.no_grad():
        im, z_sum, alpha, median, _, _, _ = fused.rasterize_median_depth(g, T, cam, use_sh_precompute=True, background_rgb=bg,
                                                                        **args)
        d = median if depth == "median" else z_sum / alpha
        d = torch.where(alpha < 0.5, torch.zeros_like(d), d)
        by_hand.integrate(d, T, cam, im, near_thresh=0.3)
    assert torch.equal(image, im) and torch.equal(bits(fused_depth), bits(d))
    for a, b in ((vol.tsdf, by_hand.tsdf), (vol.weight, by_hand.weight), (vol.color, by_hand.color)):
        assert torch.equal(bits(a), bits(b))
    share = float((vol.weight > 0).float().mean())
    assert share > 0.02 and float((alpha >= 0.5).float().mean()) > 0.02
    assert not image.requires_grad and not vol.tsdf.requires_grad
    v, f, c = vol.extract_mesh()
    report(f"integrate_frame[{depth}]", nodes_seen=share, vertices=len(v), faces=len(f))
    assert c.shape == v.shape
