"""Per-Gaussian contribution statistics: gs_render_contributions, fused.rasterize_contributions and
DensityController.prune / prune_by_contribution against tests/contributions_ref.py (held to the existing float64
reference by tests/test_contributions_ref.py on the CPU).

Rules:
  kernel and frame   num_splats_per_pixel and pixel_count equal to the reference's; ref64.r_measure of weight_max and of
                     weight_sum with env = |the formulas in fp32 - the formulas in fp64| <= R_MAX = 8 (the standing
                     forward rule, tests/test_gpu_render_ref64.py); rows no pixel uses keep their bits
  anchor             a Gaussian alone in its tile's list has T = 1, so its weights ARE the depth kernel's alpha map:
                     weight_max equal to the map's maximum bit for bit, pixel_count to its non-zero pixels, weight_sum to
                     the fp32 sum within 256 x 2^-24 relative (at most 256 positive addends in any order)
  accumulation       a second call doubles the count, keeps the maximum's bits and moves the sum by the first call's
                     value within one rounding per atomic (a row gets one atomic per tile that lists its Gaussian)
  pruning            survivors bit for bit; pruning the Gaussians with pixel_count == 0 leaves the image of the same
                     camera bit for bit

Measured on an MI355X (every case leaves its figures in the parity report):
  kernels, eight scenes   r_sum 0.11 (opaque_stack) to 0.33 (faint_300), r_max 0.15 (opaque_stack) to 1.34 (long_1100),
                          the same figures at 64 and at 256 entries per step; pixel_count exact
  frame, shift -5.5       r_sum 0.20, r_max 0.48; 1 fragile pixel, no pixel walked otherwise; 5536 of 12000 touched
  frame, shift 0          r_sum 0.33, r_max 0.42; 186 fragile pixels, 9 of them walked otherwise than the reference's
                          own stop (with the reference's own walk: nine rows' pixel_count off by one, r_sum 2.7)
  pruning                 N = 4000 at 64 x 48: 2768 Gaussians reach no pixel and go with the image unchanged bit for
                          bit; the median weight_max (0.0022) as threshold removes 615 more, PSNR against the full
                          image 69.0 dB (reported, not asserted)"""
import functools
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.densify import DensifyConfig, DensityController
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene
from gaussian_splatting_amd.train_ops import Adam

from . import contributions_ref as C
from . import render_ref64 as R
from .helpers import report
from .ref64 import r_measure
from .test_gpu_render_ref64 import FRAME, R_MAX

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCENES = list(R.render_scenes())
NAMES = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
# what the buffers hold before a call that must leave unused rows alone.  The sum's is small against every sum a used row
# can have (one weight is at least 1e-4 / 255 = 3.9e-7), so that adding to it costs a used row one rounding of its sum
# and `got - sentinel` can be held to the reference (against 3.0 the rounding alone would be 2^-23 absolute)
SUM_SENTINEL, COUNT_SENTINEL = 2.0 ** -30, 1000


# ---- 1. the kernel against the reference ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def staged(name):
    """scene `name` on the device: packed records, lists and the colour forward's num_splats_per_pixel; once"""
    sc = R.render_scenes()[name]
    c = lambda x: x.to(DEV).float().contiguous() if x.is_floating_point() else x.to(DEV).contiguous()
    V, W, H = sc.V, sc.W, sc.H
    nty = (H + 15) // 16
    s, p = _hip.current_stream(), _hip.ptr
    uv, opacity, conic, rgb = c(sc.uv), c(sc.opacity), c(sc.conic), c(sc.coeff16[:, :, 0])
    ranges, sorted_g, bg = c(sc.ranges), c(sc.sorted_g), c(sc.bg)
    packed = torch.empty(V, 12, device=DEV)
    _hip.call("gs_pack_splats", p(uv), p(opacity), p(conic), p(rgb), V, p(packed), _hip.GS_F32, s)
    image = torch.zeros(H, W, 3, device=DEV)
    fw = torch.zeros(H, W, device=DEV)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    _hip.call("gs_render_tiles_packed", p(packed), p(rgb), None, p(ranges), p(sorted_g), p(bg), W, H, 1, 0, nty, p(nsp),
              p(fw), p(image), _hip.GS_F32, None, s)
    torch.cuda.synchronize()
    return SimpleNamespace(sc=sc, V=V, W=W, H=H, nty=nty, packed=packed, ranges=ranges, sorted_g=sorted_g, nsp=nsp)


def contributions(st, wsum, wmax, count, row_index=None, rows=None):
    """gs_render_contributions of a staged scene into the given buffers (None: NULL)"""
    p = _hip.ptr
    row0, row1 = rows if rows is not None else (0, st.nty)
    _hip.call("gs_render_contributions", p(st.packed), p(st.ranges), p(st.sorted_g), p(st.nsp), p(row_index), st.W, st.H,
              row0, row1, p(wsum), p(wmax), p(count), _hip.current_stream())


def fresh(n, sentinels=False):
    wsum = torch.full((n,), SUM_SENTINEL if sentinels else 0.0, device=DEV)
    wmax = torch.zeros(n, device=DEV)
    count = torch.full((n,), COUNT_SENTINEL if sentinels else 0, dtype=torch.int32, device=DEV)
    return wsum, wmax, count


@functools.lru_cache(maxsize=None)
def plain(name):
    """the three statistics of scene `name` from zeroed buffers, on the CPU; once, do not modify"""
    st = staged(name)
    bufs = fresh(st.V)
    contributions(st, *bufs)
    return tuple(b.cpu() for b in bufs)


def measures(wsum, wmax, ref):
    """r of the two float statistics over the rows the reference has a pixel for"""
    used = ref.pixel_count > 0
    n = int(used.sum())
    pick = lambda x: x.double().cpu()[used].reshape(n, 1)
    return dict(r_sum=r_measure(pick(wsum), pick(ref.weight_sum), pick(ref.env_sum)),
                r_max=r_measure(pick(wmax), pick(ref.weight_max), pick(ref.env_max)))


@pytest.mark.parametrize("chunk", [64, 256])
@pytest.mark.parametrize("name", SCENES)
def test_kernel_against_the_reference(name, chunk):
    """both instantiations of the kernel (64 entries staged per step: the one that runs; 256: the measurement's other
    arm, gs_debug_contributions_chunk)"""
    st, ref = staged(name), C.reference(name)
    assert int(ref.fragile.sum()) == 0
    assert torch.equal(st.nsp.cpu(), ref.nsp)
    wsum, wmax, count = fresh(st.V, sentinels=True)
    before = _hip.lib().gs_debug_contributions_chunk(chunk)
    try:
        contributions(st, wsum, wmax, count)
    finally:
        assert _hip.lib().gs_debug_contributions_chunk(before) == chunk
    wsum, wmax, count = wsum.cpu(), wmax.cpu(), count.cpu()
    used = ref.pixel_count > 0
    # rows no pixel uses keep the pattern they held, bit for bit
    assert bool((wsum[~used] == SUM_SENTINEL).all()) and bool((count[~used] == COUNT_SENTINEL).all())
    assert not wmax[~used].any()
    assert torch.equal((count - COUNT_SENTINEL).long(), ref.pixel_count)
    psum, pmax, pcount = plain(name)   # (zeroed buffers, the instantiation that runs)
    assert torch.equal(pcount.long(), ref.pixel_count) and not psum[~used].any() and torch.equal(wmax, pmax)
    vals = measures(wsum.double() - SUM_SENTINEL, wmax, ref)
    vals["r_sum_zeroed"] = measures(psum, pmax, ref)["r_sum"]
    vals.update(chunk=chunk, used=int(used.sum()), V=st.V)
    report(f"contributions_kernel[{name}, chunk {chunk}]", **vals)
    print(f"contributions_kernel[{name}, chunk {chunk}]: {vals}")
    assert vals["r_sum"] <= R_MAX and vals["r_max"] <= R_MAX, vals


# ---- 2. the bit-exact anchor to the depth kernel --------------------------------------------------------------------
def test_weights_are_the_depth_kernels_alpha():
    W, H = 48, 16
    uv = torch.tensor([[6.3, 7.9], [24.0, 8.0], [41.7, 3.2]])
    conic = torch.tensor([[5.0, 1.0, 4.0], [3.0, -1.5, 6.0], [8.0, 2.0, 2.5]])
    opacity = torch.tensor([[0.9], [0.55], [0.3]])
    ranges = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=DEV)
    sorted_g = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    s, p = _hip.current_stream(), _hip.ptr
    d_uv, d_op, d_conic = uv.to(DEV), opacity.to(DEV), conic.to(DEV)
    rgb, bg = torch.full((3, 3), 0.5, device=DEV), torch.zeros(3, device=DEV)
    packed = torch.empty(3, 12, device=DEV)
    _hip.call("gs_pack_splats", p(d_uv), p(d_op), p(d_conic), p(rgb), 3, p(packed), _hip.GS_F32, s)
    image, fw = torch.zeros(H, W, 3, device=DEV), torch.zeros(H, W, device=DEV)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    _hip.call("gs_render_tiles_packed", p(packed), p(rgb), None, p(ranges), p(sorted_g), p(bg), W, H, 1, 0, 1, p(nsp),
              p(fw), p(image), _hip.GS_F32, None, s)
    xyz_cam = torch.ones(3, 3, device=DEV)
    depth, alpha, t_end = (torch.zeros(H, W, device=DEV) for _ in range(3))
    _hip.call("gs_render_zalpha", p(packed), p(xyz_cam), p(ranges), p(sorted_g), p(nsp), W, H, 0, 1, p(depth), p(alpha),
              p(t_end), s)
    wsum, wmax, count = fresh(3)
    _hip.call("gs_render_contributions", p(packed), p(ranges), p(sorted_g), p(nsp), None, W, H, 0, 1, p(wsum), p(wmax),
              p(count), s)
    alpha = alpha.cpu()
    for g in range(3):
        a = alpha[:, 16 * g:16 * g + 16]
        assert int((a > 0).sum()) > 20, g   # (the Gaussian covers a good part of its tile)
        assert torch.equal(wmax.cpu()[g], a.max()), g
        assert int(count[g]) == int((a > 0).sum()), g
        exact = float(a.double().sum())
        assert abs(float(wsum[g]) - exact) <= 256 * 2.0 ** -24 * exact, (g, float(wsum[g]), exact)


# ---- 3. accumulation, indexing, rows --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["partial_48x40", "strip_70x13"])
def test_accumulation_indexing_and_rows(name):
    st, ref = staged(name), C.reference(name)
    V = st.V
    psum, pmax, pcount = plain(name)
    used = pcount > 0
    assert int(used.sum()) > 10
    # a second call into the same buffers
    bufs = fresh(V)
    contributions(st, *bufs)
    first = bufs[0].cpu().double()
    contributions(st, *bufs)
    wsum, wmax, count = (b.cpu() for b in bufs)
    assert torch.equal(count, 2 * pcount) and torch.equal(wmax, pmax)
    # one rounding per atomic: a row that t tiles list took t - 1 roundings of at most 2^-24 s to become `first`, and the
    # second call adds its t partial sums to a value of at most 2 s, t roundings of at most 2^-24 2 s
    bound = 3 * ref.tiles_of.double() * 2.0 ** -24 * first
    assert bool(((wsum.double() - 2 * first).abs() <= bound).all())
    assert bool((wsum[used] > first.float()[used]).all())
    # row_index: a seeded permutation into a larger buffer
    N = V + 29
    gen = torch.Generator().manual_seed(17)
    rows = torch.randperm(N, generator=gen)[:V].int()
    wsum, wmax, count = fresh(N, sentinels=True)
    d_rows = rows.to(DEV)
    contributions(st, wsum, wmax, count, row_index=d_rows)
    wsum, wmax, count = wsum.cpu(), wmax.cpu(), count.cpu()
    image_of = torch.zeros(N, dtype=torch.bool)
    image_of[rows.long()] = True
    assert torch.equal(count[rows.long()] - COUNT_SENTINEL, pcount) and torch.equal(wmax[rows.long()], pmax)
    assert bool((count[~image_of] == COUNT_SENTINEL).all()) and not wmax[~image_of].any()
    assert bool((wsum[~image_of] == SUM_SENTINEL).all())
    assert bool((wsum[rows.long()][~used] == SUM_SENTINEL).all())
    # tile rows [0, a) then [a, n) into one buffer: the whole frame's count and maximum
    if st.nty > 1:
        bufs = fresh(V)
        contributions(st, *bufs, rows=(0, 1))
        assert bool((bufs[2].cpu() <= pcount).all()) and bool((bufs[2].cpu() < pcount).any())
        contributions(st, *bufs, rows=(1, st.nty))
        assert torch.equal(bufs[2].cpu(), pcount) and torch.equal(bufs[1].cpu(), pmax)
        assert measures(bufs[0], bufs[1], ref)["r_sum"] <= R_MAX
    # each output NULL in turn leaves the other two as before
    for skip in range(3):
        bufs = list(fresh(V))
        bufs[skip] = None
        contributions(st, *bufs)
        if skip != 2:
            assert torch.equal(bufs[2].cpu(), pcount), skip
        if skip != 1:
            assert torch.equal(bufs[1].cpu(), pmax), skip
        if skip != 0:
            assert measures(bufs[0], pmax, ref)["r_sum"] <= R_MAX, skip
            if st.sc.ranges.numel() == 2:
                assert torch.equal(bufs[0].cpu(), psum), skip


def test_entry_point_validates():
    """GS_EINVAL with a message for bad arguments -- also with all three outputs NULL, which otherwise launches nothing
    and is GS_OK; empty lists touch nothing"""
    st = staged("partial_33x17")
    lib, s, p = _hip.lib(), _hip.current_stream(), _hip.ptr
    z = torch.zeros(4, device=DEV)
    zi = torch.zeros(4, dtype=torch.int32, device=DEV)
    call = lib.gs_render_contributions
    assert call(None, p(zi), None, p(zi), None, 0, 16, 0, 1, p(z), p(z), p(zi), s) == _hip.GS_EINVAL
    assert b"non-empty" in lib.gs_last_error()
    assert call(None, p(zi), None, p(zi), None, 16, 16, 0, 2, p(z), p(z), p(zi), s) == _hip.GS_EINVAL
    assert b"tile row" in lib.gs_last_error()
    assert call(None, None, None, p(zi), None, 16, 16, 0, 1, p(z), p(z), p(zi), s) == _hip.GS_EINVAL
    assert b"NULL" in lib.gs_last_error()
    assert call(None, p(zi), None, None, None, 16, 16, 0, 1, p(z), p(z), p(zi), s) == _hip.GS_EINVAL
    args = (p(st.packed), p(st.ranges), p(st.sorted_g), p(st.nsp), None, st.W, st.H)
    assert call(*args, 0, st.nty, None, None, None, s) == _hip.GS_OK
    assert call(*args, 0, st.nty + 1, None, None, None, s) == _hip.GS_EINVAL
    assert call(*args, 1, 1, p(z), p(z), p(zi), s) == _hip.GS_OK   # no tile rows: nothing to do
    # empty lists, V == 0
    W, H = 33, 17
    ranges = torch.zeros(3 * 2 + 1, dtype=torch.int32, device=DEV)
    nsp = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    e = torch.empty(0, device=DEV)
    wsum, wmax, count = fresh(4, sentinels=True)
    _hip.call("gs_render_contributions", p(e), p(ranges), p(e), p(nsp), None, W, H, 0, 2, p(wsum), p(wmax), p(count), s)
    torch.cuda.synchronize()
    assert bool((wsum == SUM_SENTINEL).all()) and not wmax.any() and bool((count == COUNT_SENTINEL).all())
    assert not z.any() and not zi.any()


# ---- 4. the frame ---------------------------------------------------------------------------------------------------
BG = FRAME["bg"]


def frame_inputs(shift, seed=FRAME["seed"]):
    c = FRAME
    g, cam, T = make_scene(c["N"], c["W"], c["H"], 0, seed=seed, device=DEV)
    g.opacity.add_(shift)
    return g, cam, T, torch.full((3,), BG, device=DEV)


def frame_stats(g, T, cam, bg, stats=None):
    return fused.rasterize_contributions(g, T, cam, use_sh_precompute=True, background_rgb=bg, stats=stats, **DEFAULTS)


def second_camera(T):
    """the frame's camera moved a little sideways and back"""
    T2 = T.clone()
    T2[0, 3] += 0.15
    T2[2, 3] += 0.1
    return T2


@pytest.mark.parametrize("shift", [FRAME["shift"], 0.0])
def test_frame(shift):
    """fused.rasterize_contributions on the 70 x 45 frame (shift -5.5: lists beyond 2 x 1024, the prefix repair runs;
    shift 0: pixels saturate): image and culling_mask those of fused.rasterize, the statistics by rule 1 against the
    reference on the frame's own complete lists, culled rows zero, two cameras into one record.

    Unlike the eight scenes the frame has fragile pixels (shift 0: 186 of 3150, whose accumulated opacity passes within
    2^-21 of 0.9999; the colour forward's fp32 stop differs from the float64 one at 9 of them, which moves nine
    Gaussians' pixel_count by one).  Where to stop is the colour forward's decision and an INPUT of the statistics
    kernel (num_splats_per_pixel), so the check is: the frame's num_splats_per_pixel equals the reference's on every
    pixel that is not fragile (as tests/test_gpu_depth_alpha.py has it), and the statistics satisfy rule 1 -- count
    exact, r <= R_MAX, every row -- against the reference that walks each pixel as far as the frame did.  With no
    differing pixel that is the reference's own walk."""
    W, H, N = FRAME["W"], FRAME["H"], FRAME["N"]
    g, cam, T, bg = frame_inputs(shift)
    image0, mask0, uv, aux = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, return_aux=True,
                                             **DEFAULTS)
    image1, mask1, _ = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)
    fused.last_flags(clear=True)
    seen = {}
    inner = fused.contributions_forward

    def spy(packed, ranges, sorted_g, nsp, *args):   # (the frame's num_splats_per_pixel: it is not among the outputs)
        seen["nsp"] = nsp.cpu()
        return inner(packed, ranges, sorted_g, nsp, *args)

    fused.contributions_forward = spy
    try:
        image, stats, mask = frame_stats(g, T, cam, bg)
    finally:
        fused.contributions_forward = inner
    flags = fused.last_flags()
    assert torch.equal(image, image1) and torch.equal(mask, mask1) and torch.equal(mask, mask0)
    assert not image.requires_grad and stats.frames == 1 and stats.n == N
    cpu = lambda x: x.detach().cpu().contiguous()
    ref = C.contributions(cpu(uv), cpu(aux["opacity"]), cpu(aux["conic"]), cpu(aux["tile_ranges"]).int(),
                          cpu(aux["sorted_gaussians"]).int(), W, H, walk=seen["nsp"])
    differs = seen["nsp"] != ref.nsp
    assert not (differs & ~ref.fragile).any()
    max_list = int((cpu(aux["tile_ranges"])[1:] - cpu(aux["tile_ranges"])[:-1]).max())
    if shift == FRAME["shift"]:
        assert max_list > 2 * 1024 and int(ref.nsp.max()) > 2 * 1024
        assert flags is not None and int(flags.sum()) > 0   # tiles ran out of the ordered prefix and were repaired
    else:
        assert int(ref.nsp.max()) < max_list
    vis = cpu(aux["vis_idx"]).long()
    culled = cpu(mask).bool()
    assert vis.numel() == N - int(culled.sum())
    wsum, wmax, count = cpu(stats.weight_sum), cpu(stats.weight_max), cpu(stats.pixel_count)
    assert not wsum[culled].any() and not wmax[culled].any() and not count[culled].any()
    assert torch.equal(stats.touched.cpu(), count > 0)
    vals = dict(V=vis.numel(), max_list=max_list, fragile_pixels=int(ref.fragile.sum()),
                pixels_walked_otherwise=int(differs.sum()), touched=int((count > 0).sum()))
    vals.update(measures(wsum[vis], wmax[vis], ref))
    report(f"contributions_frame[shift {shift}]", **vals)
    print(f"contributions_frame[shift {shift}]: {vals}")
    assert torch.equal(count[vis].long(), ref.pixel_count), vals
    assert vals["r_sum"] <= R_MAX and vals["r_max"] <= R_MAX, vals
    # culled rows are exactly zero: the same camera with the far plane at the median depth (this frame culls nothing)
    far = float(aux["xyz_camera_frame"][:, 2].median())
    d = dict(DEFAULTS, far_thresh=far)
    _, near_half, mask_far = fused.rasterize_contributions(g, T, cam, use_sh_precompute=True, background_rgb=bg, **d)
    culled_far = mask_far.bool()
    assert N // 4 < int(culled_far.sum()) < 3 * N // 4
    assert not near_half.weight_sum[culled_far].any() and not near_half.weight_max[culled_far].any()
    assert not near_half.pixel_count[culled_far].any() and bool(near_half.touched.any())
    # two cameras into one record = the two separate results combined
    T2 = second_camera(T)
    _, other, _ = frame_stats(g, T2, cam, bg)
    _, both, _ = frame_stats(g, T2, cam, bg, stats=stats)
    assert both is stats and both.frames == 2 and other.frames == 1
    assert bool((other.pixel_count.cpu() != count).any())
    assert torch.equal(both.pixel_count.cpu(), count + other.pixel_count.cpu())
    assert torch.equal(both.weight_max.cpu(), torch.maximum(wmax, other.weight_max.cpu()))
    exact = wsum.double() + other.weight_sum.cpu().double()
    # one rounding per atomic: the second view reaches a row through at most `tiles` atomics, each rounding a value of at
    # most `exact`, and `other` formed its own sum with as many
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    assert bool(((both.weight_sum.cpu().double() - exact).abs() <= 2 * tiles * 2.0 ** -24 * exact).all())


def test_frame_with_nothing_visible():
    g, cam, T, bg = frame_inputs(0.0)
    image, stats, mask = fused.rasterize_contributions(g, T, cam, 0.1, 0.2, 100, 3.0, True, bg)
    assert bool(mask.all()) and bool((image == BG).all())
    assert stats.frames == 1 and not stats.weight_sum.any() and not stats.weight_max.any() and not stats.pixel_count.any()
    assert not stats.touched.any()


def test_frame_antialiased():
    """antialiased=True: the image of fused.rasterize(antialiased=True), and the weights carry the compensated opacity
    (no larger than the classic ones anywhere, smaller somewhere)"""
    g, cam, T, bg = frame_inputs(0.0)
    want, _, _ = fused.rasterize(g, T, cam, use_sh_precompute=True, background_rgb=bg, antialiased=True, **DEFAULTS)
    image, stats, _ = fused.rasterize_contributions(g, T, cam, use_sh_precompute=True, background_rgb=bg,
                                                    antialiased=True, **DEFAULTS)
    _, classic, _ = frame_stats(g, T, cam, bg)
    assert torch.equal(image, want)
    assert bool(stats.touched.any()) and bool((stats.weight_max != classic.weight_max).any())
    front = classic.weight_max.argmax()   # (the largest weight of the frame is a first contributor's: T = 1, w = alpha)
    assert float(stats.weight_max[front]) < float(classic.weight_max[front])


# ---- 5. pruning -----------------------------------------------------------------------------------------------------
LRS = (2e-4, 4e-3, 1e-2, 2e-2, 4e-3, 2e-4)


def trained(N=4000, W=64, H=48, seed=31):
    g, cam, T = make_scene(N, W, H, 0, seed=seed, device=DEV)
    params = [getattr(g, k) for k in NAMES if getattr(g, k) is not None]
    for q in params:
        q.requires_grad_(True)
    opt = Adam([{"params": q, "lr": lr} for q, lr in zip(params, LRS)])
    gen = torch.Generator(device=DEV).manual_seed(seed + 1)
    for _ in range(2):
        for q in params:
            q.grad = torch.randn(q.shape, generator=gen, device=DEV) * 1e-3
        opt.step()
    return g, cam, T, opt, DensityController(g, opt, DensifyConfig()), gen


def state_of(g, opt):
    out = {}
    for k in NAMES:
        q = getattr(g, k)
        if q is not None:
            st = opt.state[q]
            out[k] = (q.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"])
    return out


def test_prune_moves_parameters_and_moments():
    g, cam, T, opt, ctrl, gen = trained()
    N = g.xyz.shape[0]
    keep = torch.rand(N, generator=gen, device=DEV) < 0.6
    before = state_of(g, opt)
    ctrl.grad_accum_count += 3
    info = ctrl.prune(keep)
    n_keep = int(keep.sum())
    assert info == dict(deleted=N - n_keep, n_before=N, n_after=n_keep) and 0 < n_keep < N
    for i, k in enumerate(k for k in NAMES if getattr(g, k) is not None):
        q = getattr(g, k)
        assert opt.param_groups[i]["params"][0] is q and q.shape[0] == n_keep, k
        st = opt.state[q]
        old_p, old_m, old_v, old_step = before[k]
        assert torch.equal(q.detach(), old_p[keep]), k
        assert torch.equal(st["exp_avg"], old_m[keep]) and torch.equal(st["exp_avg_sq"], old_v[keep]), k
        assert float(st["step"]) == float(old_step) == 2.0, k   # the step counts are kept
    assert tuple(ctrl.uv_grad_accum.shape) == (n_keep, 2) and tuple(ctrl.xyz_grad_accum.shape) == (n_keep, 3)
    assert tuple(ctrl.grad_accum_count.shape) == (n_keep,) and not ctrl.grad_accum_count.any()
    for k in NAMES:
        q = getattr(g, k)
        if q is not None:
            q.grad = torch.randn(q.shape, generator=gen, device=DEV) * 1e-3
    held = g.xyz.detach().clone()
    opt.step()
    assert bool(torch.isfinite(g.xyz).all()) and bool((g.xyz.detach() != held).any())
    with pytest.raises(RuntimeError, match="keep must be"):
        ctrl.prune(keep)   # the mask of the old N
    assert ctrl.prune(torch.ones(n_keep, dtype=torch.bool, device=DEV))["deleted"] == 0


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * torch.log10(torch.tensor(mse)).item()


def test_prune_by_contribution():
    g, cam, T, opt, ctrl, gen = trained()
    N = g.xyz.shape[0]
    bg = torch.full((3,), BG, device=DEV)
    image, stats, mask = frame_stats(g, T, cam, bg)
    untouched = stats.pixel_count == 0
    assert int(untouched.sum()) > int(mask.sum())   # Gaussians inside the frustum that reach no pixel
    assert 0 < int(stats.touched.sum()) < N
    before = state_of(g, opt)
    info = ctrl.prune_by_contribution(stats, 0.0)
    assert info["deleted"] == int(untouched.sum()) and info["n_after"] == N - info["deleted"]
    assert torch.equal(g.xyz.detach(), before["xyz"][0][~untouched])
    # dropping entries that contribute to no pixel changes no pixel's sequence of contributors
    pruned, stats2, _ = frame_stats(g, T, cam, bg)
    assert torch.equal(pruned, image)
    assert bool(stats2.touched.all())
    assert torch.equal(stats2.weight_max, stats.weight_max[~untouched])
    assert torch.equal(stats2.pixel_count, stats.pixel_count[~untouched])
    with pytest.raises(RuntimeError, match="sweep the views again"):
        ctrl.prune_by_contribution(stats, 0.0)   # the statistics of the old N
    # a positive threshold removes strictly more
    thr = float(stats2.weight_max.median())
    n1 = g.xyz.shape[0]
    info2 = ctrl.prune_by_contribution(stats2, thr)
    assert 0 < info2["deleted"] < n1 and info2["n_after"] == int((stats2.weight_max >= thr).sum())
    smaller, _, _ = frame_stats(g, T, cam, bg)
    vals = dict(N=N, untouched=int(untouched.sum()), threshold=thr, deleted_by_threshold=info2["deleted"],
                psnr_pruned_vs_full=psnr(smaller, image))
    report("contributions_prune", **vals)
    print(f"contributions_prune: {vals}")
