"""The depth cut's kernels (csrc/binning.hip: gs_tile_count_cut, gs_tile_emit_sort_cut, the repair pass inside
gs_render_tiles_cut) array by array against tests/cut_ref.py on the CPU oracle's complete lists.

tests/test_gpu_depth_cut.py checks the cut through frames of 300 k to 3.4 M Gaussians that must come out bit-equal to
the uncut HIP frame; here the scenes have 3 000 to 12 000 Gaussians -- the smallest at which every tile is still cut,
tiles are cut and whole side by side, a tile keeps nothing, a list holds exactly 1024 entries, a repaired list
exceeds the LDS sort -- the complete lists come from the oracle, and every array the stage leaves is compared on its
own: full_ranges, totals, b*, kept ranges, bucket offsets, control words, kept lists, flags, overflow lists.  All
comparisons are exact."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene

from .cut_ref import check_bounds, cut_reference, flag_bounds, sortable
from .helpers import _oracle, report
from .ref64 import general_camera_scene, to_device
from .test_gpu_parity import extreme_footprints

pytestmark = pytest.mark.gpu
DEV = "cuda"
KCUT = 1024
COOP_MIN = 48   # binning.hip: candidate windows of more tiles are walked by a whole wave


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def synthetic(N, W, H, seed=11):
    g, cam, T = make_scene(N, W, H, 0, seed=seed)
    d = DEFAULTS
    return SimpleNamespace(g=g, cam=cam, T=T, W=W, H=H, near=d["near_thresh"], far=d["far_thresh"],
                           pad=d["cull_mask_padding"], mh=d["mh_dist"])


# ---- the driver: the three C-ABI calls of a depth-cut stage, buffers as fused._preprocess_forward_cut sizes them ----
def cut_stage(sc_or_scene, rows=None, edit=None, may_be_empty=False):
    """gs_preprocess_forward_cut, [edit(bin_rec[:V]): may overwrite columns 0-4 (u, v, conic) of the bin records in
    place], gs_tile_count_cut, gs_tile_emit_sort_cut on tile rows `rows` (default: all; the per-Gaussian stage's cut form
    serves whole frames only, the two binning calls take the band).  -> everything the stage left,
    as CPU tensors, and under .dev the device buffers gs_render_tiles_cut needs.  Asserts gs_cut_supported and that the
    depth histogram is all zero again (may_be_empty: a frame without a visible Gaussian is what the test is about)."""
    sc = sc_or_scene
    if isinstance(sc, tuple):
        g, cam, T = sc
        d = DEFAULTS
        sc = SimpleNamespace(g=g, cam=cam, T=T, W=cam.width, H=cam.height, near=d["near_thresh"], far=d["far_thresh"],
                             pad=d["cull_mask_padding"], mh=d["mh_dist"])
    lib = _hip.lib()
    g, cam, pose = to_device(sc, DEV)
    dev = g.xyz.device
    N, W, H = g.xyz.shape[0], sc.W, sc.H
    n_sh = 1 if g.sh is None else g.sh.shape[2] + 1
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    T = ntx * nty
    row0, row1 = rows if rows is not None else (0, nty)
    assert lib.gs_cut_supported(ntx, row0, row1, N), "the case must lie in the depth cut's LDS-histogram regime"
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    ws, count, rank, vis_idx = i32(lib.gs_preprocess_workspace_ints(N)), i32(1), i32(N), i32(N)
    tile_ws, ranges_buf, full_ranges = i32(lib.gs_tile_workspace_ints(T)), i32(T + 3), i32(T + 1)
    cut_ws = i32(lib.gs_cut_workspace_ints(N, T))
    culled = torch.empty(N, dtype=torch.uint8, device=dev)
    center, uv, xyz_cam, conic, opa, rgbr = f32(3), f32(N, 2), f32(N, 3), f32(N, 3), f32(N, 1), f32(N, 3)
    packed, bin_rec = f32(N, 12), f32(N, 8)
    hist = fused._depth_hist(dev)
    mh = ctypes.c_float(sc.mh)
    _hip.call("gs_preprocess_forward_cut", p(g.xyz), p(g.quaternion), p(g.scale), p(g.opacity), p(g.rgb), p(g.sh), n_sh,
              p(pose), p(cam.K), N, W, H, sc.near, sc.far, sc.pad, mh, 0, nty, p(ws), p(center), p(count), p(culled),
              p(rank), p(vis_idx), p(uv), p(xyz_cam), p(conic), p(opa), p(rgbr), p(packed), p(bin_rec), p(cut_ws), p(hist),
              lib.gs_cut_sample_stride(N), stream)
    V = int(count[0])
    assert may_be_empty or V * 8 > 1024 * (row1 - row0) * ntx, "enough visible Gaussians for the depth cut's regime"
    rec = bin_rec[:V].cpu()
    # the bin records are what the binning reads: columns 0-4 and 5 are uv, conic and z of the stage's own outputs
    assert torch.equal(rec[:, 0:2], uv[:V].cpu()) and torch.equal(rec[:, 2:5], conic[:V].cpu())
    assert torch.equal(rec[:, 5], xyz_cam[:V, 2].cpu())
    if edit is not None:
        edit(bin_rec[:V])
        rec = bin_rec[:V].cpu()
    _hip.call("gs_tile_count_cut", p(bin_rec), N, p(count), ntx, nty, mh, row0, row1, p(tile_ws), p(cut_ws), p(ranges_buf),
              p(full_ranges), None, stream)
    S_kept, V2, S_full = (int(x) for x in ranges_buf[T:T + 3].tolist())
    assert V2 == V
    keys = torch.empty(max(S_kept, 1), dtype=torch.int64, device=dev)
    sorted_g = torch.full((max(S_kept, 1),), -1, dtype=torch.int32, device=dev)
    _hip.call("gs_tile_emit_sort_cut", p(bin_rec), N, ntx, nty, mh, row0, row1, p(ranges_buf), p(tile_ws), p(cut_ws),
              p(keys), ctypes.c_int64(S_kept), p(sorted_g), stream)
    torch.cuda.synchronize()
    assert not bool(hist.any()), "the depth histogram must be all zero again on exit"
    ptrs = [ctypes.c_void_p() for _ in range(5)]
    _hip.check(lib.gs_cut_debug_views(p(cut_ws), N, T, *[ctypes.byref(x) for x in ptrs]))
    off = [(x.value - cut_ws.data_ptr()) // 4 for x in ptrs]
    view = lambda k, n: cut_ws[off[k]:off[k] + n].cpu()
    return SimpleNamespace(
        sc=sc, N=N, V=V, W=W, H=H, ntx=ntx, nty=nty, T=T, rows=(row0, row1), S_kept=S_kept, S_full=S_full, rec=rec,
        ranges=ranges_buf.cpu().long(), full_ranges=full_ranges.cpu().long(), sorted_g=sorted_g.cpu().long(),
        bstar=view(0, T).long(), totals=view(1, T).long(), bounds=view(2, 1024), boff=view(3, 1025).long(),
        ctrl=view(4, 2).long(),
        dev=SimpleNamespace(packed=packed, rgb=rgbr, uv=uv, conic=conic, opacity=opa, ranges_buf=ranges_buf, sorted_g=sorted_g,
                            full_ranges=full_ranges, bin_rec=bin_rec, tile_ws=tile_ws, cut_ws=cut_ws, stream=stream,
                            keep=(g, cam, pose, ws, rank, vis_idx, culled, center, xyz_cam, keys, count)))


def oracle_lists(st):
    """the complete lists of the frame from the CPU oracle, on the (uv, conic) the bin records hold and the stage's z"""
    rec = st.rec
    uv, conic = rec[:, 0:2].contiguous(), rec[:, 2:5].contiguous()
    xyz_c = torch.stack([torch.zeros(st.V), torch.zeros(st.V), rec[:, 5]], dim=1).contiguous()
    assert bool(torch.isfinite(rec[:, 5]).all())
    return _oracle().get_sorted_gaussian_list(1024, uv, xyz_c, conic, st.ntx, st.nty, st.sc.mh)


def check_stage(st, ref_sorted, ref_ranges):
    """every array of the stage against the restatement -> the reference"""
    T, (row0, row1) = st.T, st.rows
    whole = (row0, row1) == (0, st.nty)
    check_bounds(st.bounds, st.sc.near, st.sc.far, st.V > 0)
    ref = cut_reference(ref_ranges, ref_sorted, sortable(st.rec[:, 5]), st.bounds, KCUT, None if whole else (row0, row1), st.ntx)
    band = ref.in_band
    if whole:
        assert torch.equal(st.full_ranges, ref_ranges.long())          # complete ranges == the oracle's
    assert torch.equal(st.full_ranges, ref.full_ranges)
    assert torch.equal(st.totals[band], ref.totals[band])                   # (only the band's tiles are written)
    nonempty = band & (ref.totals > 0)
    assert torch.equal(st.bstar[nonempty], ref.bstar[nonempty])
    assert bool((st.bstar[band & (ref.totals == 0)] == -1).all())
    assert torch.equal(st.ranges[:T + 1], ref.kept_ranges)
    assert int(st.ranges[T]) == st.S_kept == int(ref.kept.sum())
    assert int(st.ranges[T + 1]) == st.V and int(st.ranges[T + 2]) == st.S_full == int(ref.totals.sum())
    assert int(st.boff[0]) == 0 and int(st.boff[1024]) == st.V
    assert torch.equal(st.boff[1:] - st.boff[:-1], ref.populations)
    assert int(st.ctrl[0]) == ref.deepest
    assert torch.equal(st.sorted_g[:st.S_kept], ref.kept_sorted)           # the kept lists, entry for entry
    assert bool((st.sorted_g[st.S_kept:] == -1).all())
    n_kept = st.ranges[1:T + 1] - st.ranges[:T]
    assert bool((n_kept[~band] == 0).all()) and bool(((st.full_ranges[1:] - st.full_ranges[:-1])[~band] == 0).all())
    assert int(n_kept.max()) <= KCUT
    return ref


def numbers(tag, st, ref, **more):
    b = ref.in_band
    trunc = b & (ref.kept < ref.totals)
    report(f"cut_lists[{tag}]", V=st.V, tiles=int(b.sum()), truncated_tiles=int(trunc.sum()),
           whole_tiles=int((b & ~trunc).sum()), kept_min=int(ref.kept[b].min()), kept_max=int(ref.kept[b].max()),
           list_min=int(ref.totals[b].min()), list_max=int(ref.totals[b].max()), S_kept=st.S_kept, S_full=st.S_full, **more)
    return trunc


# ---- scenes -----------------------------------------------------------------------------------------------------
def dense():
    return synthetic(12000, 96, 64)


def half_dense():
    sc = dense()
    x = sc.g.xyz[:, 0]
    sc.g.xyz[(x > 0) & (torch.arange(x.numel()) % 8 != 0), 2] = -1.0
    return sc


def depths(case):
    sc = synthetic(8000, 64, 48)
    z = sc.g.xyz[:, 2]
    if case == "ties":
        z[::2] = 6.0
    elif case == "one_depth":
        z.fill_(6.0)
    elif case == "two_depths":
        z.copy_(torch.where(torch.arange(z.numel()) % 2 == 0, 4.0, 9.0))
    return sc


GENERAL = {"75x53": (31, 12000, 75, 53), "11x500": (32, 12000, 11, 500), "120x13": (33, 6000, 120, 13)}


def general(name, opacity=None):
    seed, N, W, H = GENERAL[name]
    sc = general_camera_scene(seed, N, W=W, H=H, deg=0, stress=True)
    if opacity is not None:
        sc.g.opacity.fill_(opacity)
    return sc


EXACT_SIZES = (1023, 1024, 1025, 2048, 129, 0)


def place_exact(rec):
    """bin records by index into the six tiles of a 96 x 16 frame, EXACT_SIZES entries each, every footprint inside its
    tile (radius < 3 px around a centre 3 .. 13 px into the tile); the rest far off screen"""
    gen = torch.Generator().manual_seed(21)
    V = rec.shape[0]
    new = torch.zeros(V, 5)
    new[:, 0], new[:, 1] = -1e6, 8.0
    new[:, 2:5] = torch.tensor([0.5, 0.0, 0.5])
    at = 0
    for tile, n in enumerate(EXACT_SIZES):
        new[at:at + n, 0] = 16.0 * tile + 3.0 + 10.0 * torch.rand(n, generator=gen)
        new[at:at + n, 1] = 3.0 + 10.0 * torch.rand(n, generator=gen)
        at += n
    assert at <= V
    rec[:, 0:5] = new.to(rec.device)


def place_extreme(seed, W, H):
    def edit(rec):
        uv, _, conic = extreme_footprints(seed, W, H, rec.shape[0])
        rec[:, 0:2], rec[:, 2:5] = uv.to(rec.device), conic.to(rec.device)
    return edit


STAGE_CASES = {
    "dense": lambda: (dense(), None),
    "barely": lambda: (synthetic(3000, 64, 48), None),
    "half_dense": lambda: (half_dense(), None),
    "ties": lambda: (depths("ties"), None),
    "one_depth": lambda: (depths("one_depth"), None),
    "two_depths": lambda: (depths("two_depths"), None),
    "general[75x53]": lambda: (general("75x53"), None),
    "general[11x500]": lambda: (general("11x500"), None),
    "general[120x13]": lambda: (general("120x13"), None),
    "exact_1024": lambda: (synthetic(12000, 96, 16), place_exact),
    "extreme[50x40]": lambda: (synthetic(4000, 50, 40), place_extreme(5, 50, 40)),
    "extreme[160x112]": lambda: (synthetic(12000, 160, 112), place_extreme(6, 160, 112)),
    # (beyond the two above, whose lists all stay whole: truncated tiles, so that the emit's skip of a tile that is cut
    # in front of the bucket -- before the separating-axis test -- meets the extreme footprints as well)
    "extreme[50x40] truncated": lambda: (synthetic(12000, 50, 40), place_extreme(7, 50, 40)),
}


@pytest.mark.parametrize("case", list(STAGE_CASES))
def test_cut_stage_arrays_equal_the_reference(case):
    sc, edit = STAGE_CASES[case]()
    st = cut_stage(sc, edit=edit)
    ref_sorted, ref_ranges = oracle_lists(st)
    ref = check_stage(st, ref_sorted, ref_ranges)
    trunc = numbers(case, st, ref)
    n_trunc, n_whole = int(trunc.sum()), int((~trunc).sum())
    # what the case is there for (conditions on the oracle's lists and the restatement, not on the kernels)
    if case == "dense" or case.startswith("general"):
        assert n_whole == 0, "every tile truncated"
    if case == "barely":
        assert n_trunc >= 1 and n_whole >= 1
    if case == "half_dense":
        assert n_trunc >= 4 and n_whole >= 4
    if case == "ties":
        assert n_whole == 0 and int(ref.kept.max()) < 512, "every tile truncated in front of the tie bucket"
    if case == "one_depth":
        long = ref.totals > KCUT
        assert int(long.sum()) > 0 and bool((ref.bstar[long] == -1).all()) and bool((ref.kept[long] == 0).all())
        assert st.S_kept == 0, "nothing is kept: the emit has nothing to write"
    if case == "exact_1024":
        assert ref.totals.tolist() == list(EXACT_SIZES)
        assert ref.kept[:2].tolist() == [1023, 1024] and ref.kept[5] == 0
        assert bool((ref.kept[2:4] < ref.totals[2:4]).all()) and bool((ref.kept[2:4] <= KCUT).all())
        assert int(ref.kept[4]) == 129
    if case.startswith("extreme"):
        hits = torch.bincount(ref_sorted.long(), minlength=st.V)
        if case == "extreme[160x112]":
            assert int(hits.max()) > COOP_MIN, "a footprint wide enough for the wave-cooperative walk"
        if case.endswith("truncated"):
            assert n_trunc >= 4
        assert not bool(torch.isfinite(st.rec[:, 0:5]).all()), "non-finite footprints are part of the case"


@pytest.mark.parametrize("rows", [(1, 3), (0, 1), (3, 4)])
def test_cut_stage_of_a_tile_row_band(rows):
    """the t0 / Tb arguments of the cut kernels: the band's tiles as in the whole frame, every other tile empty"""
    st = cut_stage(dense(), rows=rows)
    ref_sorted, ref_ranges = oracle_lists(st)
    ref = check_stage(st, ref_sorted, ref_ranges)
    whole = cut_reference(ref_ranges, ref_sorted, sortable(st.rec[:, 5]), st.bounds, KCUT)
    b = ref.in_band
    assert int(b.sum()) == (rows[1] - rows[0]) * st.ntx and int(ref.totals[~b].sum()) == 0
    assert torch.equal(ref.kept[b], whole.kept[b]) and torch.equal(st.bstar[b], whole.bstar[b])
    numbers(f"dense rows {rows[0]}-{rows[1]}", st, ref)


def test_everything_culled_frame_leaves_empty_lists_and_a_zero_histogram():
    sc = synthetic(3000, 64, 48)
    sc.g.xyz[:, 2] = -1.0
    st = cut_stage(sc, may_be_empty=True)
    assert st.V == 0 and st.S_kept == 0 and st.S_full == 0
    ref_sorted, ref_ranges = oracle_lists(st)
    ref = check_stage(st, ref_sorted, ref_ranges)
    assert ref.deepest == -1 and not bool(st.ranges.any()) and not bool(st.boff.any())
    assert bool((st.bounds == -1).all())   # no sample: every boundary all ones


# ---- repair lists and flags: one render per case through gs_render_tiles_cut ---------------------------------------
def cut_render(st):
    """gs_render_tiles_cut on the stage's buffers, overflow list pre-filled with -1 -> flags, overflow_sorted, image,
    num_splats, final weight (CPU) and the flag counter ctrl[1]"""
    d, dev = st.dev, st.dev.packed.device
    W, H, T = st.W, st.H, st.T
    image = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    fw = torch.empty(H, W, dtype=torch.float32, device=dev)
    nsp = torch.empty(H, W, dtype=torch.int32, device=dev)
    flags, cost = torch.full((T,), -1, dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.int32, device=dev)
    cap = max(st.S_full, 1)
    okeys = torch.empty(cap, dtype=torch.int64, device=dev)
    osorted = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    bg = torch.full((3,), 0.5, device=dev)
    _hip.call("gs_render_tiles_cut", p(d.packed), p(d.rgb), p(d.ranges_buf), p(d.sorted_g), ctypes.c_int64(st.S_kept),
              p(d.full_ranges), p(d.bin_rec), st.N, ctypes.c_float(st.sc.mh), p(d.tile_ws), p(d.cut_ws), p(okeys), p(osorted),
              ctypes.c_int64(st.S_full), p(bg), W, H, 0, st.nty, p(flags), p(nsp), p(fw), p(image), p(cost), None, d.stream)
    torch.cuda.synchronize()
    ptrs = [ctypes.c_void_p() for _ in range(5)]
    _hip.check(_hip.lib().gs_cut_debug_views(p(d.cut_ws), st.N, T, *[ctypes.byref(x) for x in ptrs]))
    ctrl1 = int(d.cut_ws[(ptrs[4].value - d.cut_ws.data_ptr()) // 4 + 1])
    return SimpleNamespace(flags=flags.cpu().long(), osorted=osorted.cpu().long(), image=image.cpu(), nsp=nsp.cpu(),
                           fw=fw.cpu(), flagged_count=ctrl1)


def oracle_render(st, ref_sorted, ref_ranges):
    """the oracle's fp32 render of the COMPLETE lists, from the stage's own per-splat values"""
    d, V = st.dev, st.V
    c = lambda x: x[:V].cpu().contiguous()
    img = torch.zeros(st.H, st.W, 3)
    nsp = torch.zeros(st.H, st.W, dtype=torch.int32)
    fw = torch.zeros(st.H, st.W)
    _oracle().render_tiles_cuda(c(d.uv), c(d.opacity), c(d.rgb), c(d.conic), torch.zeros(1, 1, 1), ref_ranges, ref_sorted,
                                torch.full((3,), 0.5), nsp, fw, img)
    return img, nsp, fw


def faint_left():
    sc = dense()
    sc.g.opacity[sc.g.xyz[:, 0] < 0] = -5.5
    return sc


def faint(sc):
    sc.g.opacity.fill_(-5.0)
    return sc


RENDER_CASES = {
    "dense": dense,
    "dense half faint": faint_left,
    "dense faint": lambda: faint(dense()),
    "one_depth": lambda: depths("one_depth"),
    "general[11x500] faint": lambda: general("11x500", opacity=-5.0),
}


@pytest.mark.parametrize("case", list(RENDER_CASES))
def test_flags_and_repair_lists_equal_the_reference(case):
    st = cut_stage(RENDER_CASES[case]())
    ref_sorted, ref_ranges = oracle_lists(st)
    ref = check_stage(st, ref_sorted, ref_ranges)
    got = cut_render(st)
    img, nsp, fw = oracle_render(st, ref_sorted, ref_ranges)
    must, may = flag_bounds(ref.kept, ref.totals, nsp, st.W, st.H)
    flags = got.flags != 0
    deepest = int(nsp.max())
    longest = int(ref.totals[flags].max()) if bool(flags.any()) else 0
    numbers(case + ", render", st, ref, flagged_tiles=int(flags.sum()), must_flag=int(must.sum()), may_flag=int(may.sum()),
            deepest_pixel=deepest, longest_repaired_list=longest)
    assert bool(((got.flags == 0) | (got.flags == 1)).all())
    assert bool((flags | ~must).all()), "a truncated tile with a pixel deeper than its prefix must be flagged"
    assert bool((may | ~flags).all()), "only truncated tiles that reach the end of their prefix may be flagged"
    assert got.flagged_count == int(flags.sum())
    # the overflow buffer: the oracle's complete list for every flagged tile, untouched everywhere else
    fr = ref_ranges.long()
    expect = torch.full_like(got.osorted, -1)
    for t in torch.nonzero(flags).flatten().tolist():
        expect[fr[t]:fr[t + 1]] = ref_sorted.long()[fr[t]:fr[t + 1]]
    assert torch.equal(got.osorted, expect)
    # the header's promise: the results are those of the complete lists, bit for bit
    assert torch.equal(got.nsp, nsp)
    assert torch.equal(got.image, img)
    assert torch.equal(got.fw, fw)
    if case == "dense half faint":
        assert 0 < int(flags.sum()) < st.T
    if case == "one_depth":
        assert bool((ref.kept[flags] == 0).all()) and int(flags.sum()) > 0, "repaired from an empty prefix"
    if case == "general[11x500] faint":
        assert longest > 8192, "a repaired list beyond the LDS sort"
