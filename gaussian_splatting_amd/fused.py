"""Fast path with the contract of splat_py.rasterize.rasterize (reference: splat_py/rasterize.py:18-112):

    image, culling_mask, uv = rasterize(gaussians, camera_T_world, camera, near_thresh, far_thresh,
                                        cull_mask_padding, mh_dist, use_sh_precompute, background_rgb)

Two autograd nodes instead of six-plus-glue:

    _Preprocess   gs_preprocess_forward + tile binning + per-tile sort   (parameters -> uv, conic,
                  opacity, colour)
    _Render       gs_render_tiles_prefix (_packed) / gs_render_tiles_backward_slab (_abs: rasterize(absgrad=True))

Both get the frame record (_frame_record) as a non-tensor argument: the frame's options from the entry point and, after
_Preprocess.forward, what is not differentiable (packed records, tile lists, culling mask, an early render).  Every entry
point starts with the same prelude (_begin_frame: refuse, validate, make contiguous, _Preprocess).  So `uv` is still an autograd intermediate between two nodes: `uv.retain_grad()` followed by
`uv.grad` gives the render-backward grad_uv exactly as the trainer expects (trainer.py:360,379).
One small device->host read per frame (V and S, to size the outputs); the reference has ~25
synchronisation points.  fp32, SH-precompute colour mode; anything else is routed
to the reference-shaped path in splat_py.rasterize (still HIP kernels, never a CPU fallback).

The four stages are plain functions (preprocess_forward, render_forward, render_backward,
preprocess_backward) that gaussian_splatting_amd.sharded composes differently for multi-GPU frames.

rasterize_rgbd is the same frame with two more differentiable outputs, depth and accumulated opacity [H, W]
(_Render with the map policy _DepthMap: gs_render_zalpha / gs_render_zalpha_backward next to the colour kernels,
gs_z_backward behind the per-Gaussian backward).  rasterize_distortion adds the depth-distortion map of
the same walk as a fourth output (_DistortionMap: gs_render_distortion / gs_render_distortion_backward in place of the
depth kernels).

rasterize_features composites caller-supplied per-Gaussian feature vectors [N, C <= 32] with the frame's weights into a
differentiable [H, W, C] map next to the image and the accumulated opacity (_Render with the map policy _FeatureMap:
gs_render_features / gs_render_features_backward).

filter3d= on the entry points is Mip-Splatting's 3D smoothing filter: per-Gaussian world-space variances
that the per-Gaussian stage adds to the covariance and compensates in the opacity, forward and backward
(gs_preprocess_forward_filtered and its two backward twins).  filter3d_rate / filter3d_from_rate make the filter from the
training cameras (gs_filter3d_rate), bake_filter3d folds it into the parameters for export.

rasterize_normals is the feature frame with the channels filled in for the normal-consistency regulariser:
_GaussianNormals (gs_gaussian_normals / gs_gaussian_normals_backward) forms the visible Gaussians' normals, the feature
walk composites (n_x, n_y, n_z, z) into a normal map and the depth map.  depth_to_normal (_DepthNormal: gs_depth_normal /
gs_depth_normal_backward) is the other side of that loss, the normal of a rendered depth map.
"""
import os
from types import SimpleNamespace

import torch

from . import _hip
from .splat_py import rasterize as _reference_shaped
from .splat_py.structs import TILE_EDGE_LENGTH_PX
from .splat_py.utils import compute_rays_in_world_frame


_p = _hip.ptr


def _stream():
    # every stage asks once and passes it on
    return _hip.current_stream()


# Prefix mode of the per-tile sort (include/gsplat_hip.h: gs_tile_emit_sort): order only the 1024
# nearest entries of long tile lists and repair, on the device, the tiles that needed more.  Exact;
# off only for callers that want the complete sorted lists back (return_aux=True).
SORT_PREFIX = True
# mean tile-list length from which the backward starts its tiles longest-first (render_backward)
LPT_MIN_MEAN_LIST = 256
# Enqueue the render on the speculative tile lists before waiting for the frame's host read.
EARLY_RENDER = True

# Depth cut (csrc/binning.hip "depth cut"; include/gsplat_hip.h): the count pass walks the Gaussians in depth buckets,
# every tile learns the last bucket up to which it holds <= 1024 entries, and only those are emitted and sorted; a
# truncated tile that runs out of list unsaturated is repaired on the device from its complete list.  Exact.
# "auto": whole frames in the LDS-histogram regime whose lists averaged DEPTH_CUT_MIN_MEAN_LIST entries or more in
# an earlier frame of the same shape (the partition of the Gaussians by depth costs ~0.03 ms: it must buy more than
# that); True / False force it.  Callers that want the complete lists back (return_aux) never get it.
DEPTH_CUT = {"0": False, "1": True}.get(os.environ.get("GSPLAT_DEPTH_CUT", "auto"), "auto")   # (env: A/B runs of bench.py)
DEPTH_CUT_MIN_MEAN_LIST = 1280
_mean_list_hint = {}   # frame shape -> complete instance count of the latest frame

last_tile_flags = None   # int32[T] of the latest prefix-mode frame of the Python path (see last_flags())
# Frames without hooks go through the native orchestration (csrc/frame_hip.cpp: the same C-ABI calls and
# autograd structure in C++, one Python call per frame).  False = always the Python orchestration below.
NATIVE = True
_native_mod = None
_native_failed = False


def native():
    """the gsplat_frame module, or None when NATIVE is off / it is not built (the Python orchestration of
    the same HIP kernels is then used; this is a host-side speed-up, not a compute fallback)"""
    global _native_mod, _native_failed
    if not NATIVE or _native_failed:
        return None
    if _native_mod is None:
        try:
            from . import splat_cuda_native
            _native_mod = splat_cuda_native.load_frame()
            _hip.timing_providers.append(_native_mod)
        except ImportError as e:
            import warnings
            _native_failed = True
            warnings.warn(f"native frame orchestration unavailable ({e}); using the Python orchestration")
            return None
    return _native_mod


def last_flags(clear=False):
    """tile_flags (int32[T]; 1 = the prefix sort ran out and the tile was repaired) of the latest
    prefix-mode frame, whichever orchestration ran it; None if there was none since the last clear"""
    global last_tile_flags
    out = last_tile_flags
    m = _native_mod
    if m is not None:
        nat = m.last_tile_flags(clear)
        out = nat if nat is not None else out
    if clear:
        last_tile_flags = None
    return out


# fused.keep_last_slab: ONE slot for the [V, 9] slab of the latest per-Gaussian backward, whichever orchestration ran
# it -- inside the native module when that is loaded (its backward runs without the interpreter), else _last_slab
_keep_slab = False
_last_slab = None
_last_grad_z = None   # rasterize_rgbd frames: dL/dz [V] of the visible Gaussians, kept with the slab
_last_grad_normals = None   # rasterize_normals frames: dL/dn [V, 3] of the visible Gaussians' normals, kept with the slab
_slab_slot = None   # the native module holding the slot, fixed by keep_last_slab(True)


def keep_last_slab(on):
    """Tests and tools: while on, both orchestrations keep a reference (no copy) to the render-gradient slab of their
    latest per-Gaussian backward.  The render backward's summation order differs from run to run, so a gradient
    derived from the slab (camera_T_world's) can only be checked against the slab it was computed from.  Every call
    drops what was kept."""
    global _keep_slab, _last_slab, _slab_slot, _last_grad_z, _last_grad_normals
    _keep_slab, _last_slab, _last_grad_z, _last_grad_normals = bool(on), None, None, None
    if _native_mod is not None:
        _native_mod.keep_last_slab(False)
    _slab_slot = native() if on else None
    if _slab_slot is not None:
        _slab_slot.keep_last_slab(True)


def last_slab():
    """the [V, 9] slab (rgb 3 | opacity 1 | uv 2 | conic 3) of the latest per-Gaussian backward since
    keep_last_slab(True), whichever orchestration ran it; None if there was none"""
    return _slab_slot.last_slab() if _slab_slot is not None else _last_slab


def last_grad_z():
    """dL/dz [V] (z = xyz_camera_frame[:, 2]) that the latest rasterize_rgbd backward since keep_last_slab(True) handed
    to the per-Gaussian node next to the slab; None if that frame's depth went unused or there was none"""
    return _last_grad_z


def last_grad_normals():
    """dL/dn [V, 3] that the latest rasterize_normals backward since keep_last_slab(True) handed to the normals' node
    (what gs_gaussian_normals_backward and the pose's rotation term were computed from); None if there was none"""
    return _last_grad_normals


def _note_slab(slab, V):
    global _last_slab
    if _slab_slot is not None:
        _slab_slot.note_slab(slab[:V])
    else:
        _last_slab = slab[:V]


_capacity_hint = {}   # (device, N, tiles, band) -> instance capacity guessed from the previous frame
_pinned = {}

SLAB_WIDTH = 9   # render gradients per visible Gaussian: rgb 3 | opacity 1 | uv 2 | conic 3
SLAB_RGB, SLAB_OPACITY, SLAB_UV, SLAB_CONIC = slice(0, 3), slice(3, 4), slice(4, 6), slice(6, 9)


_PINNED_RING = 4   # host read buffers per (device, size): frames in flight on other streams / threads keep their own


def _pinned_ints(dev, n):
    """a pinned int32[n] for the frame's host read, from a small ring: a frame whose read is still
    pending (another stream or thread) does not see its record overwritten by the next frame"""
    ring = _pinned.get((dev.index, n))
    if ring is None:
        ring = _pinned[(dev.index, n)] = [[torch.empty(n, dtype=torch.int32, pin_memory=True) for _ in range(_PINNED_RING)], 0]
    ring[1] = (ring[1] + 1) % _PINNED_RING
    return ring[0][ring[1]]


# ---- frame counters (bench.py --moving-camera reports them) ---------------------------------------------
_counters = {"frames": 0, "speculative_frames": 0, "capacity_misses": 0, "S_min": None, "S_max": None,
             "depth_cut_frames": 0}
_flag_log = []   # tile_flags of recent prefix-mode frames (device tensors: summed only when counters() is asked)


def reset_counters():
    _counters.update(frames=0, speculative_frames=0, capacity_misses=0, S_min=None, S_max=None, depth_cut_frames=0)
    _flag_log.clear()
    if _native_mod is not None:
        _native_mod.reset_counters()


def counters():
    """frames seen since reset_counters(): how many were enqueued on a guessed capacity, how many of those
    had to repeat emit + sort + render because the instance count exceeded the guess, the range of S, and
    the tiles the prefix sort had to repair (flag-and-redo on the device).  Synchronises."""
    out = dict(_counters)
    out["prefix_repaired_tiles"] = int(sum(int(f.sum()) for f in _flag_log)) if _flag_log else 0
    out["prefix_frames_logged"] = len(_flag_log)
    out["orchestration"] = "python"
    if _native_mod is not None:
        nat = _native_mod.counters()
        if nat["frames"]:
            out["depth_cut_backoffs"] = nat.get("depth_cut_backoffs", 0)
            for k in ("prefix_frames_without_repair_launches", "prefix_late_repairs", "long_list_misses"):
                out[k] = nat.get(k, 0)
            for k in ("frames", "speculative_frames", "capacity_misses", "prefix_repaired_tiles", "prefix_frames_logged",
                      "depth_cut_frames"):
                out[k] += nat[k]
            lo = [x for x in (out["S_min"], nat["S_min"]) if x is not None]
            hi = [x for x in (out["S_max"], nat["S_max"]) if x is not None]
            out["S_min"], out["S_max"] = (min(lo) if lo else None), (max(hi) if hi else None)
            out["orchestration"] = "native (csrc/frame_hip.cpp)" if nat["frames"] == out["frames"] else "mixed"
    return out


class _Arena:
    """one allocation cut into 1-D blocks of the given element counts, each starting 16-byte aligned"""

    def __init__(self, dtype, device, sizes, zero=False):
        self.offsets, off = [], 0
        for n in sizes:
            self.offsets.append((off, n))
            off += (n + 3) & ~3
        self.buf = (torch.zeros if zero else torch.empty)(off, dtype=dtype, device=device)

    def blocks(self):
        return [self.buf[o:o + n] for o, n in self.offsets]


# ---------------------------------------------------------------------------------------------------
# stages
# ---------------------------------------------------------------------------------------------------
def _tile_grid(width, height):
    """-> (n_tiles_x, n_tiles_y) of a width x height image"""
    return ((width + TILE_EDGE_LENGTH_PX - 1) // TILE_EDGE_LENGTH_PX,
            (height + TILE_EDGE_LENGTH_PX - 1) // TILE_EDGE_LENGTH_PX)


def want_depth_cut(hint_key, N, ntx, row0, row1, whole):
    """the "auto" policy of DEPTH_CUT for one frame"""
    if DEPTH_CUT is False or not whole:
        return False
    if not _hip.lib().gs_cut_supported(ntx, row0, row1, N):
        return False
    if DEPTH_CUT is True:
        return True
    n_tiles = (row1 - row0) * ntx
    known = _mean_list_hint.get(hint_key, 0)
    if known < DEPTH_CUT_MIN_MEAN_LIST * n_tiles:
        return False
    # "auto" cut and "auto" segments exclude each other per shape: a cut frame takes the unsegmented backward, so a
    # small dense frame would change backward kernels (and the last bits of its gradients) whenever the cut policy
    # switches; such shapes keep the segments.  What counts is the choice segments_for() STORED for the shape when
    # there is one; segments forced on (SEGMENTS = True) keep the auto cut off -- a cut frame cannot honour them
    # (csrc/frame_hip.cpp want_depth_cut does the same)
    if SEGMENTS != "auto":
        return not bool(SEGMENTS)
    if hint_key in _segment_choice:
        return not _segment_choice[hint_key]
    return not want_segments(known, n_tiles)


CAMERA_MODELS = ("pinhole", "fisheye")


def _raster_mode(antialiased, camera_model):
    """-> the raster_mode bit mask of the C ABI's _mode entries; a camera_model that is neither name raises RuntimeError"""
    if camera_model not in CAMERA_MODELS:
        raise RuntimeError(f"camera_model must be one of {' / '.join(repr(m) for m in CAMERA_MODELS)}, "
                           f"got {camera_model!r}")
    return ((_hip.GS_RASTER_ANTIALIASED if antialiased else _hip.GS_RASTER_CLASSIC)
            | (_hip.GS_RASTER_FISHEYE if camera_model == "fisheye" else 0))


def preprocess_forward(xyz, quaternion, scale, opacity, rgb, sh, camera_T_world, K, width, height, near_thresh,
                       far_thresh, cull_mask_padding, mh_dist, tile_rows, sort_prefix, plan=None, plan_ints=0,
                       defer=False, depth_cut=False, antialiased=False, camera_model="pinhole", filter3d=None):
    """Per-Gaussian stage, binning and per-tile sort of one frame.  filter3d: float32 [N] world-space variances of the 3D
    smoothing filter (gs_preprocess_forward_filtered; whole frames, combines with the two below); None: the call without
    it (the entry then launches what gs_preprocess_forward_mode launches).  antialiased: the packed record's opacity carries the
    factor sqrt(det Sigma_2D / det(Sigma_2D + 0.25 I)) (gs_preprocess_forward_mode, GS_RASTER_ANTIALIASED; whole frames).
    camera_model: "pinhole", or "fisheye" -- uv, the cull and the projection Jacobian of the equidistant fisheye model
    (GS_RASTER_FISHEYE; whole frames, combines with antialiased).  `plan`, if given, is called as
    plan(f) after the per-Gaussian stage is enqueued and fills the device record f.record
    (plan_ints int32) that rides on the frame's one host read (its host copy is left in f.host:
    multi-GPU, the split sizes of the gradient exchange); it may set f.subset = (index list, device
    count) to restrict the binning to those rows.  defer=True returns before the host read: the caller may enqueue the render on
    the speculative lists (f.sorted_buf, f.keys_buf, f.capacity) and calls preprocess_finish(f)."""
    dev = xyz.device
    N = xyz.shape[0]
    n_sh = 1 if sh is None else sh.shape[2] + 1
    ntx, nty = _tile_grid(width, height)
    T = ntx * nty
    row0, row1 = tile_rows if tile_rows is not None else (0, nty)
    f = SimpleNamespace(N=N, n_sh=n_sh, ntx=ntx, nty=nty, T=T, row0=row0, row1=row1, width=width, height=height,
                        mh_dist=mh_dist, sort_prefix=sort_prefix, antialiased=bool(antialiased),
                        camera_model=camera_model, raster_mode=_raster_mode(antialiased, camera_model), filter3d=filter3d)
    _require(not (filter3d is not None and tile_rows is not None), "filter3d serves whole frames: tile_rows is not supported")
    _require(not (antialiased and tile_rows is not None), "antialiased=True serves whole frames: tile_rows is not supported")
    _require(not (camera_model == "fisheye" and tile_rows is not None),
             'camera_model="fisheye" serves whole frames: tile_rows is not supported')

    stream = f.stream = _stream()
    f.hint_key = (dev.index, N, T, row0, row1)
    if depth_cut:
        assert plan is None and not defer, "the depth cut is a single-GPU, whole-frame path in the Python orchestration"
        return _preprocess_forward_cut(f, xyz, quaternion, scale, opacity, rgb, sh, camera_T_world, K, near_thresh,
                                       far_thresh, cull_mask_padding)
    # two allocations for the stage's buffers (host time matters at ~1 ms per frame): an int32 arena
    # for the bookkeeping and a float32 arena for the per-Gaussian outputs, blocks 16-byte aligned
    n_ws = _hip.lib().gs_preprocess_workspace_ints(N)
    n_tc = _hip.lib().gs_tile_workspace_ints(T)
    iar = _Arena(torch.int32, dev, (n_ws, 1, N, N, n_tc, T + 2 + plan_ints, (N + 3) // 4))
    f.ws, f.count, f.rank, f.vis_idx, f.tile_counts, f.ranges_buf, mask_bytes = iar.blocks()
    f.culling_mask = mask_bytes.view(torch.bool)[:N]   # kernel writes 0/1 bytes
    far = _Arena(torch.float32, dev, (3, 2 * N, 3 * N, 3 * N, N, 3 * N, 12 * N))
    f.center, uv, xyz_cam, conic, opa, rgbr, packed = far.blocks()
    f.uv, f.xyz_cam, f.conic = uv.view(N, 2), xyz_cam.view(N, 3), conic.view(N, 3)
    f.opacity_act, f.rgb_render, f.packed = opa.view(N, 1), rgbr.view(N, 3), packed.view(N, 12)
    f.cut = None
    _hip.call("gs_preprocess_forward_filtered", _p(xyz), _p(quaternion), _p(scale), _p(opacity),
              _p(rgb), _p(sh), n_sh, _p(camera_T_world), _p(K), N, width, height, near_thresh, far_thresh,
              cull_mask_padding, mh_dist, row0, row1, _p(f.ws), _p(f.center), _p(f.count), _p(f.culling_mask), _p(f.rank),
              _p(f.vis_idx), _p(f.uv), _p(f.xyz_cam), _p(f.conic), _p(f.opacity_act), _p(f.rgb_render), _p(f.packed),
              None, None, None, 0, _p(filter3d), f.raster_mode, stream, label="gs_preprocess_forward")

    # the plan's record lives right behind (S, V) at the tail of ranges_buf: one host read gets both
    f.subset = (None, None)
    f.record = f.ranges_buf[T + 2:]
    if plan is not None:
        plan(f)
    subset, subset_n = f.subset
    _hip.call("gs_tile_count", _p(f.uv), _p(f.conic), N, _p(f.count), _p(subset), _p(subset_n), ntx, nty,
              mh_dist, row0, row1, _p(f.tile_counts), _p(f.ranges_buf), None, stream)

    # The frame's only device->host read: (S, V) [+ the plan's record], to size the outputs.  If a
    # previous frame of the same shape is known, the emit + sort are enqueued first with a capacity
    # guessed from it, so the GPU keeps working while the host waits for the integers; the kernels
    # never write beyond the capacity and the step is repeated only if S turned out larger.
    guess = _capacity_hint.get(f.hint_key)
    f.host_buf = _pinned_ints(dev, 2 + plan_ints)

    def read_back(non_blocking):
        f.host_buf.copy_(f.ranges_buf[T:], non_blocking=non_blocking)

    f.ranges = f.ranges_buf[:T + 1]
    f.speculative = guess is not None
    if f.speculative:
        read_back(True)
        f.ready = torch.cuda.Event()
        f.ready.record()
        f.capacity = guess
    else:
        read_back(False)
        f.capacity = int(f.host_buf[0])
    f.sorted_buf, f.keys_buf = _emit_sort(f, f.capacity)
    f.deferred = defer
    if not defer:
        preprocess_finish(f)
    return f


def _emit_sort(f, capacity):
    """-> the sorted lists and keys of stage record f in buffers of `capacity` instances (gs_tile_emit_sort).  (A plain
    function of f: a closure kept on f would tie the record to itself, and the frame's arenas to the cyclic collector.)"""
    dev = f.uv.device
    sorted_buf = torch.empty(capacity, dtype=torch.int32, device=dev)
    keys = torch.empty(capacity, dtype=torch.int64, device=dev)
    if capacity > 0:
        subset, subset_n = f.subset
        _hip.call("gs_tile_emit_sort", _p(f.uv), _p(f.xyz_cam), _p(f.conic), f.N, _p(f.count), _p(subset),
                  _p(subset_n), f.ntx, f.nty, f.mh_dist, f.row0, f.row1, _p(f.ranges_buf), _p(f.tile_counts), _p(keys),
                  capacity, _p(sorted_buf), f.sort_prefix, f.stream)
    return sorted_buf, keys


_DEPTH_HIST = {}


def _depth_hist(dev):
    """the depth histogram gs_preprocess_forward_cut fills and returns to zero: one per (device, stream), zeroed once"""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    if key not in _DEPTH_HIST:
        _DEPTH_HIST[key] = torch.zeros(_hip.GS_CUT_HIST_BINS, dtype=torch.int32, device=dev)
    return _DEPTH_HIST[key]


def _preprocess_forward_cut(f, xyz, quaternion, scale, opacity, rgb, sh, camera_T_world, K, near_thresh, far_thresh,
                            cull_mask_padding):
    """preprocess_forward with the depth-bucketed binning (DEPTH_CUT).  The Python orchestration of this mode reads
    the frame's counts before it emits (no speculative capacity): it serves tests and tools; frames without hooks
    run through csrc/frame_hip.cpp."""
    lib = _hip.lib()
    dev = xyz.device
    N, T, ntx, nty, row0, row1 = f.N, f.T, f.ntx, f.nty, f.row0, f.row1
    stream = f.stream
    stride = lib.gs_cut_sample_stride(N)
    n_ws = lib.gs_preprocess_workspace_ints(N)
    n_tc = lib.gs_tile_workspace_ints(T)
    n_cut = lib.gs_cut_workspace_ints(N, T)
    iar = _Arena(torch.int32, dev, (n_ws, 1, N, N, n_tc, T + 3, (N + 3) // 4, n_cut, T + 1))
    f.ws, f.count, f.rank, f.vis_idx, f.tile_counts, f.ranges_buf, mask_bytes, cut_ws, full_ranges = iar.blocks()
    f.culling_mask = mask_bytes.view(torch.bool)[:N]
    far = _Arena(torch.float32, dev, (3, 2 * N, 3 * N, 3 * N, N, 3 * N, 12 * N, 8 * N))
    f.center, uv, xyz_cam, conic, opa, rgbr, packed, bin_rec = far.blocks()
    f.uv, f.xyz_cam, f.conic = uv.view(N, 2), xyz_cam.view(N, 3), conic.view(N, 3)
    f.opacity_act, f.rgb_render, f.packed = opa.view(N, 1), rgbr.view(N, 3), packed.view(N, 12)
    _hip.call("gs_preprocess_forward_filtered", _p(xyz), _p(quaternion), _p(scale), _p(opacity),
              _p(rgb), _p(sh), f.n_sh, _p(camera_T_world), _p(K), N, f.width, f.height, near_thresh, far_thresh,
              cull_mask_padding, f.mh_dist, row0, row1, _p(f.ws), _p(f.center), _p(f.count), _p(f.culling_mask),
              _p(f.rank), _p(f.vis_idx), _p(f.uv), _p(f.xyz_cam), _p(f.conic), _p(f.opacity_act), _p(f.rgb_render),
              _p(f.packed), _p(bin_rec), _p(cut_ws), _p(_depth_hist(dev)), stride, _p(f.filter3d),
              f.raster_mode, stream, label="gs_preprocess_forward")
    _hip.call("gs_tile_count_cut", _p(bin_rec), N, _p(f.count), ntx, nty, f.mh_dist, row0, row1,
              _p(f.tile_counts), _p(cut_ws), _p(f.ranges_buf), _p(full_ranges), None, stream)
    f.subset = (None, None)
    f.record = f.ranges_buf[T + 3:]
    f.host_buf = _pinned_ints(dev, 3)
    f.host_buf.copy_(f.ranges_buf[T:T + 3])
    S, V, S_full = (int(x) for x in f.host_buf.tolist())
    sorted_buf = torch.empty(S, dtype=torch.int32, device=dev)
    keys = torch.empty(S, dtype=torch.int64, device=dev)
    if S > 0:
        _hip.call("gs_tile_emit_sort_cut", _p(bin_rec), N, ntx, nty, f.mh_dist, row0, row1, _p(f.ranges_buf),
                  _p(f.tile_counts), _p(cut_ws), _p(keys), S, _p(sorted_buf), stream)
    c = _counters
    c["frames"] += 1
    c["depth_cut_frames"] += 1
    c["S_min"] = S_full if c["S_min"] is None else min(c["S_min"], S_full)
    c["S_max"] = S_full if c["S_max"] is None else max(c["S_max"], S_full)
    _mean_list_hint[f.hint_key] = S_full
    f.ranges = f.ranges_buf[:T + 1]
    f.speculative, f.deferred, f.capacity = False, False, S
    f.sorted_buf = f.sorted_g = sorted_buf
    f.keys_buf = f.keys = keys
    f.S, f.V, f.host = S, V, []
    f.cut = SimpleNamespace(bin_rec=bin_rec, cut_ws=cut_ws, full_ranges=full_ranges, S_full=S_full, N=N,
                            tile_counts=f.tile_counts, mh_dist=f.mh_dist, flags=None, overflow_sorted=None)
    return f


def preprocess_finish(f):
    """Waits for the frame's host read and fixes the sizes (f.S, f.V, f.sorted_g, f.keys, f.host).
    -> True if the speculative capacity was too small and emit + sort were repeated (anything
    enqueued on the speculative lists in between has to be repeated too)."""
    redone = False
    if f.speculative:
        f.ready.synchronize()
    S, V = int(f.host_buf[0]), int(f.host_buf[1])
    c = _counters
    c["frames"] += 1
    c["speculative_frames"] += int(f.speculative)
    c["S_min"] = S if c["S_min"] is None else min(c["S_min"], S)
    c["S_max"] = S if c["S_max"] is None else max(c["S_max"], S)
    if S > f.capacity:
        f.sorted_buf, f.keys_buf = _emit_sort(f, S)
        f.capacity = S
        redone = True
        c["capacity_misses"] += 1
    # the capacity only sizes two buffers (12 B per instance; the kernels write S entries whatever it is), so
    # the guess is the largest count seen for this frame shape plus a margin: views of a training run
    # differ by tens of percent in S, and a miss costs a repeated emit + sort + render
    _capacity_hint[f.hint_key] = max(_capacity_hint.get(f.hint_key, 0), int(S * 1.25) + 4096)
    _mean_list_hint[f.hint_key] = S
    f.host = f.host_buf.tolist()[2:]
    f.S, f.V = S, V
    f.sorted_g = f.sorted_buf[:S]
    f.keys = f.keys_buf[:S]   # prefix mode: the repair pass of the render sorts flagged tiles from these
    return redone


def preprocess_backward(xyz, quaternion, scale, camera_T_world, K, f, slab, v_base=0, i0=0, i1=None, antialiased=False,
                        camera_model="pinhole", filter3d=None):
    """Dense parameter gradients of the Gaussians [i0, i1) from the render-gradient slab
    (row of visible Gaussian v at slab[v - v_base]).  xyz, quaternion, scale: the full tensors.
    antialiased: the slab's opacity column is the gradient of the antialiased opacity (gs_preprocess_backward_mode).
    camera_model: the model the forward projected with (the uv and conic columns go back through it).
    filter3d: the full [N] filter the forward ran with (gs_preprocess_backward_filtered), or None."""
    mode = _raster_mode(antialiased, camera_model)
    i1 = f.N if i1 is None else i1
    n = i1 - i0
    dev = xyz.device
    n_extra = 3 * (f.n_sh - 1)
    gx, gq, gs, go, gc, gsh = _Arena(torch.float32, dev, (3 * n, 4 * n, 3 * n, n, 3 * n, n_extra * n)).blocks()
    grad_xyz, grad_q, grad_scale = gx.view(n, 3), gq.view(n, 4), gs.view(n, 3)
    grad_opacity, grad_rgb = go.view(n, 1), gc.view(n, 3)
    grad_sh = gsh.view(n, 3, f.n_sh - 1) if f.n_sh > 1 else None
    if n > 0:
        _hip.call("gs_preprocess_backward_filtered", _p(xyz[i0:i1]), _p(quaternion[i0:i1]),
                  _p(scale[i0:i1]), f.n_sh, _p(camera_T_world), _p(K), _p(f.center), _p(f.rank[i0:i1]), _p(f.opacity_act),
                  _p(slab), v_base, n, _p(grad_xyz), _p(grad_q), _p(grad_scale), _p(grad_opacity), _p(grad_rgb),
                  _p(grad_sh), _p(filter3d[i0:i1] if filter3d is not None else None), mode, _stream(), label="gs_preprocess_backward")
    return grad_xyz, grad_q, grad_scale, grad_opacity, grad_rgb, grad_sh


def pose_backward(xyz, quaternion, scale, camera_T_world, K, f, slab, v_base=0, antialiased=False,
                  camera_model="pinhole", filter3d=None):
    """The gradient of camera_T_world [4, 4] from the render-gradient slab of frame record f (gs_pose_backward): the
    rotation block and the translation as twelve free numbers, the last row 0.  Reads the quaternion and scale the
    forward saw: with the fused optimizer step it goes BEFORE preprocess_backward_adam on the same stream."""
    n = f.N
    mode = _raster_mode(antialiased, camera_model)
    # (two allocations: the gradient outlives the backward, the workspace must not live as long)
    grad = torch.empty(4, 4, dtype=torch.float32, device=xyz.device)
    ws = torch.empty(_hip.lib().gs_pose_workspace_floats(n), dtype=torch.float32, device=xyz.device)
    # (antialiased: the opacity column reaches the pose through the factor's conic terms, which need the sigmoid)
    opacity_act = f.opacity_act if mode & _hip.GS_RASTER_ANTIALIASED else None
    _hip.call("gs_pose_backward_filtered", _p(xyz), _p(quaternion), _p(scale), _p(camera_T_world),
              _p(K), _p(f.rank), _p(opacity_act), _p(slab), v_base, n, _p(ws), _p(grad), _p(filter3d), mode,
              _stream(), label="gs_pose_backward")
    return grad


def preprocess_backward_adam(xyz, camera_T_world, K, f, slab, plan):
    """preprocess_backward with the optimizer step folded in (gs_preprocess_backward_adam): -> grad_xyz only;
    quaternion, scale, opacity, rgb and sh are stepped in place with their moments, no gradient is written for them.
    plan.begin() -> ([(param, exp_avg, exp_avg_sq, lr, step) x 5, sh's entry None without SH], beta1, beta2, eps):
    called here, i.e. at backward time, after the node has unpacked its saved tensors (train_ops.FusedRasterAdam)."""
    rows, beta1, beta2, eps = plan.begin()
    n = f.N
    grad_xyz = torch.empty(n, 3, dtype=torch.float32, device=xyz.device)
    if n > 0:
        args = []
        for r in rows:
            p, m, v, lr, step = r if r is not None else (None, None, None, 0.0, 1)
            args += [_p(p), _p(m), _p(v), lr, step]
        _hip.call("gs_preprocess_backward_adam", _p(xyz), f.n_sh, _p(camera_T_world), _p(K), _p(f.center), _p(f.rank),
                  _p(f.opacity_act), _p(slab), 0, n, _p(grad_xyz), *args, beta1, beta2, eps, _stream())
        # the kernel wrote through raw pointers: bump the version counters like an in-place torch op would
        for r in rows:
            if r is not None:
                for t in r[:3]:
                    torch.autograd.graph.increment_version(t)
    return grad_xyz


# Depth segments of the backward (csrc/render.hip "depth segments"): the forward leaves, per (tile, 128-entry
# segment of its list, pixel), the state a backward walk has at the segment boundary, and the backward runs one
# workgroup per (tile, segment).  "auto": for frames / bands of fewer than SEGMENT_MAX_TILES tiles whose lists
# average SEGMENT_MIN_MEAN_LIST entries or more -- a multi-GPU rank's band is two workgroups per CU otherwise.
# Measured at workload D, forward + backward: 1/8 band 0.259 -> 0.205 ms (backward 0.173 -> 0.093, the forward pays
# 0.086 -> 0.112 for the extra state), 1/4 band 0.321 -> 0.298, half frame 0.463 -> 0.489: on below 1500 tiles.
# True / False force it.
SEGMENTS = "auto"
SEGMENT_MAX_TILES = 1500
SEGMENT_MIN_MEAN_LIST = 192
_EMPTY = {}


def _empty(dev, dtype=torch.float32):
    key = (dev, dtype)
    if key not in _EMPTY:
        _EMPTY[key] = torch.empty(0, dtype=dtype, device=dev)
    return _EMPTY[key]


def want_segments(n_instances, n_tiles):
    if SEGMENTS == "auto":
        return 0 < n_tiles < SEGMENT_MAX_TILES and n_instances >= SEGMENT_MIN_MEAN_LIST * n_tiles
    return bool(SEGMENTS) and n_tiles > 0


_segment_choice = {}   # frame shape (the capacity hint's key) -> "auto"'s decision, fixed by the first exact count


def segments_for(hint_key, n_instances, exact_count, n_tiles):
    """want_segments, decided once per frame shape: a speculative frame only knows a capacity (1.25 S + 4096), so
    near the threshold the first frame and the later frames of one scene would otherwise pick different backward
    kernels (gradients differing in the last bits from frame to frame)."""
    if SEGMENTS != "auto":
        return want_segments(n_instances, n_tiles)
    if hint_key in _segment_choice:
        return _segment_choice[hint_key]
    on = want_segments(n_instances, n_tiles)
    if exact_count:
        _segment_choice[hint_key] = on
    return on


def render_forward(packed, rgb, ranges, sorted_g, keys, background_rgb, height, width, tile_rows, sort_prefix,
                   image_rows=None, segments=None, cut=None):
    """cut: the frame's depth-cut record (preprocess_forward(depth_cut=True).cut) -> gs_render_tiles_cut.
    -> image, splat counts, final weights, tile costs, segment state.  image_rows > height: the image buffer
    gets that many rows (the multi-GPU gather wants equal-sized bands); the kernels only see the first `height`.
    tile costs: int32[n_tiles], how long each tile took (prefix mode; empty otherwise) -- the launch-order
    hint render_backward hands back to the library.  segment state: the workspace for the depth-segmented
    backward (empty when segments are off; `segments` None = the module's policy), for render_backward."""
    dev = packed.device
    ntx, nty = _tile_grid(width, height)
    row0, row1 = tile_rows if tile_rows is not None else (0, nty)
    # one allocation: image [H,W,3] | final weight [H,W] | splat count [H,W] (int32 view).  Rows outside
    # [row0, row1) are not written by the kernel: zero-fill only when sharded
    alloc = torch.empty if tile_rows is None else torch.zeros
    P = height * width
    PI = (image_rows if image_rows is not None else height) * width
    buf = alloc(3 * PI + 2 * P, dtype=torch.float32, device=dev)
    image = buf[:3 * PI].view(-1, width, 3)
    fw = buf[3 * PI:3 * PI + P].view(height, width)
    nsp = buf[3 * PI + P:].view(torch.int32).view(height, width)
    stream = _stream()
    if segments is None:
        segments = want_segments(sorted_g.shape[0], (row1 - row0) * ntx)
    seg = _empty(dev)
    if segments:
        seg = torch.empty(_hip.lib().gs_render_segment_workspace_bytes(width, height, row0, row1) // 4,
                          dtype=torch.float32, device=dev)
    seg_p = _p(seg) if segments else None
    if cut is None and not (sort_prefix and sorted_g.shape[0] > sort_prefix):
        cost = _empty(dev, torch.int32)
        _hip.call("gs_render_tiles_packed", _p(packed), _p(rgb), None, _p(ranges), _p(sorted_g), _p(background_rgb),
                  width, height, 1, row0, row1, _p(nsp), _p(fw), _p(image), _hip.GS_F32, seg_p, stream)
        return image, nsp, fw, cost, seg
    # cut and prefix lists: a provisional render, whose tiles that ran out of list are flagged and rendered again
    # from their complete lists -- one call, the host never looks at the flags
    scratch = torch.empty(2 * ntx * nty, dtype=torch.int32, device=dev)
    flags, cost = scratch[:ntx * nty], scratch[ntx * nty:]
    if cut is not None:
        # depth-cut lists (preprocess_forward(depth_cut=True)): kept prefixes first, flagged tiles repaired from
        # their complete lists in the overflow buffers
        assert not segments, "depth segments and the depth cut are not combined"
        # (never empty: a frame without a visible Gaussian still hands the backward a non-null overflow list)
        okeys = torch.empty(max(cut.S_full, 1), dtype=torch.int64, device=dev)
        osorted = torch.empty(max(cut.S_full, 1), dtype=torch.int32, device=dev)
        _hip.call("gs_render_tiles_cut", _p(packed), _p(rgb), _p(ranges), _p(sorted_g), sorted_g.shape[0],
                  _p(cut.full_ranges), _p(cut.bin_rec), cut.N, cut.mh_dist, _p(cut.tile_counts), _p(cut.cut_ws),
                  _p(okeys), _p(osorted), cut.S_full, _p(background_rgb), width, height, row0, row1,
                  _p(flags), _p(nsp), _p(fw), _p(image), _p(cost), None, stream)
        cut.flags, cut.overflow_sorted = flags, osorted
    else:
        # the ordered prefixes; flagged tiles are sorted in full from `keys`
        _hip.call("gs_render_tiles_prefix", _p(packed), _p(rgb), _p(ranges), _p(sorted_g), _p(keys),
                  sorted_g.shape[0], _p(background_rgb), width, height, row0, row1, _p(flags),
                  _p(nsp), _p(fw), _p(image), _p(cost), seg_p, stream)
    global last_tile_flags
    last_tile_flags = flags
    if len(_flag_log) < 512:
        _flag_log.append(flags)
    return image, nsp, fw, cost, seg


def render_backward(packed, rgb, ranges, sorted_g, background_rgb, nsp, fw, grad_image, height, width, tile_rows,
                    V, tile_cost=None, backward_mode=None, seg_state=None, cut=None, tail=0, uv_absgrad=None):
    """-> the slab [V, 9] of accumulated render gradients (rgb 3 | opacity 1 | uv 2 | conic 3).
    tail > 0 (rasterize_rgbd): -> (slab, float[tail]); the tail lies behind the slab's rows in the same allocation and
    is cleared by the same prologue launch.  grad_image None: the slab is cleared and no colour backward runs.
    tile_cost: render_forward's fourth output (the tiles are then started longest-first).
    seg_state: render_forward's fifth output; non-empty -> one workgroup per (tile, depth segment).
    backward_mode: _hip.GS_BACKWARD_COMPAT / _EXACT, per call (ABI 5); None = the process default at the call
    uv_absgrad: float32 [max(V, 1), 2] -> cleared here, and the colour backward is gs_render_tiles_backward_slab_abs
    (ABI 18), which next to the slab leaves there the per-pixel magnitudes of the uv gradient's terms (AbsGS); the same
    walk under the same order / segment / cut arguments"""
    nty = _tile_grid(width, height)[1]
    row0, row1 = tile_rows if tile_rows is not None else (0, nty)
    # (cleared by the call itself, in the launch that also orders the tiles: zero_slab_rows)
    rows = max(V, 1)
    slab = torch.empty(rows + (tail + SLAB_WIDTH - 1) // SLAB_WIDTH, SLAB_WIDTH, dtype=torch.float32, device=packed.device)
    cost = order = None
    seg_on = seg_state is not None and seg_state.numel() > 0
    # longest-first only pays where a workgroup lives long enough for the kernel's tail to matter: lists of a
    # few hundred entries per tile (workload B, 52 per tile: the order kernel's 6 us are not won back)
    if (grad_image is not None and not seg_on and tile_cost is not None and tile_cost.numel() > 0
            and sorted_g.shape[0] >= LPT_MIN_MEAN_LIST * tile_cost.numel()):
        cost = tile_cost
        order = torch.empty(tile_cost.numel() + 8, dtype=torch.int32, device=packed.device)
    # one prologue launch (clear the slab + order the tiles), then the render kernel alone in its entry
    _hip.call("gs_render_backward_prologue", _p(slab), slab.shape[0], _p(cost), _p(order), width, height, row0, row1,
              _stream())
    if uv_absgrad is not None:
        uv_absgrad.zero_()   # the sums of THIS backward (the entry accumulates)
    if grad_image is not None:
        walk = (_p(packed), _p(rgb), _p(ranges), _p(sorted_g), _p(background_rgb),
                _p(nsp), _p(fw), _p(grad_image), width, height, row0, row1, _p(slab), 0, None, _p(order),
                _p(seg_state) if seg_on else None, _p(cut.flags) if cut is not None else None,
                _p(cut.full_ranges) if cut is not None else None, _p(cut.overflow_sorted) if cut is not None else None,
                _hip.GS_BACKWARD_DEFAULT if backward_mode is None else int(backward_mode))
        if uv_absgrad is None:
            _hip.call("gs_render_tiles_backward_slab", *walk, _stream())
        else:
            _hip.call("gs_render_tiles_backward_slab_abs", *walk, None, _p(uv_absgrad), _stream())
    if tail:
        return slab[:V], slab.view(-1)[rows * SLAB_WIDTH:rows * SLAB_WIDTH + tail]
    return slab[:V]


def zalpha_forward(packed, xyz_cam, ranges, sorted_g, nsp, height, width):
    """-> depth, alpha, T_end, each [H, W] (gs_render_zalpha): the differentiable depth and accumulated opacity of the
    frame whose colour forward left nsp; one allocation"""
    nty = _tile_grid(width, height)[1]
    buf = torch.empty(3, height, width, dtype=torch.float32, device=packed.device)
    _hip.call("gs_render_zalpha", _p(packed), _p(xyz_cam), _p(ranges), _p(sorted_g), _p(nsp), width, height, 0, nty,
              _p(buf[0]), _p(buf[1]), _p(buf[2]), _stream())
    return buf[0], buf[1], buf[2]


def zalpha_backward(packed, xyz_cam, ranges, sorted_g, nsp, t_end, grad_depth, grad_alpha, height, width, slab, grad_z):
    """adds the depth / alpha maps' gradients to columns 3..8 of the (cleared or colour-filled) slab and to grad_z
    (gs_render_zalpha_backward); either grad may be None"""
    nty = _tile_grid(width, height)[1]
    gd = grad_depth.contiguous() if grad_depth is not None else None
    ga = grad_alpha.contiguous() if grad_alpha is not None else None
    _hip.call("gs_render_zalpha_backward", _p(packed), _p(xyz_cam), _p(ranges), _p(sorted_g), _p(nsp), _p(t_end),
              _p(gd), _p(ga), width, height, 0, nty, _p(slab), _p(grad_z), _stream())


def distortion_forward(packed, xyz_cam, ranges, sorted_g, nsp, height, width):
    """-> (depth, distortion), alpha, T_end, each [H, W] (gs_render_distortion): zalpha_forward's three maps, bit for
    bit, and the depth distortion 2 sum_k w_k (z_k A_<k - D_<k) of the same walk; one allocation"""
    nty = _tile_grid(width, height)[1]
    buf = torch.empty(4, height, width, dtype=torch.float32, device=packed.device)
    _hip.call("gs_render_distortion", _p(packed), _p(xyz_cam), _p(ranges), _p(sorted_g), _p(nsp), width, height, 0, nty,
              _p(buf[3]), _p(buf[0]), _p(buf[1]), _p(buf[2]), _stream())
    return (buf[0], buf[3]), buf[1], buf[2]


def distortion_backward(packed, xyz_cam, ranges, sorted_g, nsp, t_end, depth, alpha, grad_distortion, grad_depth,
                        grad_alpha, height, width, slab, grad_z):
    """adds the distortion / depth / alpha maps' gradients to columns 3..8 of the (cleared or colour-filled) slab and
    to grad_z (gs_render_distortion_backward); depth, alpha: the forward's totals; any grad may be None"""
    nty = _tile_grid(width, height)[1]
    gx, gd, ga = (g.contiguous() if g is not None else None for g in (grad_distortion, grad_depth, grad_alpha))
    _hip.call("gs_render_distortion_backward", _p(packed), _p(xyz_cam), _p(ranges), _p(sorted_g), _p(nsp), _p(t_end),
              _p(depth), _p(alpha), _p(gx), _p(gd), _p(ga), width, height, 0, nty, _p(slab), _p(grad_z), _stream())


def median_depth_forward(packed, xyz_cam, ranges, sorted_g, nsp, height, width):
    """-> (depth, median_depth, median_index), alpha, T_end, each [H, W] (gs_render_median_depth): zalpha_forward's three
    maps, bit for bit, and from the same walk the z and the index (int32, among the visible Gaussians; -1: no
    contributor) of the entry at which the transmittance falls through 0.5; two allocations"""
    nty = _tile_grid(width, height)[1]
    buf = torch.empty(4, height, width, dtype=torch.float32, device=packed.device)
    index = torch.empty(height, width, dtype=torch.int32, device=packed.device)
    _hip.call("gs_render_median_depth", _p(packed), _p(xyz_cam), _p(ranges), _p(sorted_g), _p(nsp), width, height, 0,
              nty, _p(buf[3]), _p(index), _p(buf[0]), _p(buf[1]), _p(buf[2]), _stream())
    return (buf[0], buf[3], index), buf[1], buf[2]


def median_depth_backward(median_index, grad_median_depth, height, width, grad_z):
    """adds grad_median_depth [H, W] to grad_z at median_index (gs_median_depth_backward): the choice of entry is held
    constant, nothing goes to the slab; a None grad adds nothing"""
    nty = _tile_grid(width, height)[1]
    gm = grad_median_depth.contiguous() if grad_median_depth is not None else None
    _hip.call("gs_median_depth_backward", _p(median_index), _p(gm), width, height, 0, nty, _p(grad_z), _stream())


def features_forward(packed, feat, ranges, sorted_g, nsp, height, width):
    """-> feature_map [H, W, C], alpha, T_end [H, W] (gs_render_features) for the visible Gaussians' feature rows
    feat [V, C] on the lists of the frame whose colour forward left nsp; one allocation"""
    nty = _tile_grid(width, height)[1]
    C, P = int(feat.shape[1]), height * width
    buf = torch.empty((C + 2) * P, dtype=torch.float32, device=packed.device)
    fmap, alpha, t_end = buf[:C * P].view(height, width, C), buf[C * P:(C + 1) * P].view(height, width), \
        buf[(C + 1) * P:].view(height, width)
    _hip.call("gs_render_features", _p(packed), _p(feat), C, _p(ranges), _p(sorted_g), _p(nsp), width, height, 0, nty,
              _p(fmap), _p(alpha), _p(t_end), _stream())
    return fmap, alpha, t_end


def features_backward(packed, feat, ranges, sorted_g, nsp, t_end, grad_map, grad_alpha, height, width, slab, grad_feat):
    """adds the feature / alpha maps' gradients to columns 3..8 of the (cleared or colour-filled) slab and, unless it
    is None, to grad_feat [V, C] (gs_render_features_backward); either map gradient may be None"""
    nty = _tile_grid(width, height)[1]
    gm = grad_map.contiguous() if grad_map is not None else None
    ga = grad_alpha.contiguous() if grad_alpha is not None else None
    _hip.call("gs_render_features_backward", _p(packed), _p(feat), int(feat.shape[1]), _p(ranges), _p(sorted_g), _p(nsp),
              _p(t_end), _p(gm), _p(ga), width, height, 0, nty, _p(slab), _p(grad_feat), _stream())


def contributions_forward(packed, ranges, sorted_g, nsp, height, width, row_index=None, weight_sum=None,
                          weight_max=None, pixel_count=None):
    """adds the per-Gaussian contribution statistics of the frame whose colour forward left nsp to the given buffers
    (gs_render_contributions): weight_sum / weight_max float32, pixel_count int32, rows named by row_index (int32 [V];
    None: the visible index itself); a buffer that is None is skipped"""
    nty = _tile_grid(width, height)[1]
    _hip.call("gs_render_contributions", _p(packed), _p(ranges), _p(sorted_g), _p(nsp), _p(row_index), width, height, 0,
              nty, _p(weight_sum), _p(weight_max), _p(pixel_count), _stream())


def gaussian_normals_forward(quaternion, scale, camera_T_world, vis_idx, xyz_cam):
    """-> normals [V, 3] of the visible Gaussians in the camera frame, facing the camera (gs_gaussian_normals): column
    argmin(log-scale) of the rotation of the normalised quaternion, rotated by the pose; vis_idx int32 [V], xyz_cam [V, 3]
    as the per-Gaussian stage left them"""
    V = int(vis_idx.shape[0])
    normals = torch.empty(V, 3, dtype=torch.float32, device=quaternion.device)
    _hip.call("gs_gaussian_normals", _p(quaternion), _p(scale), _p(camera_T_world), _p(vis_idx), _p(xyz_cam), V,
              _p(normals), _stream())
    return normals


def gaussian_normals_backward(quaternion, scale, camera_T_world, rank, xyz_cam, grad_normals):
    """-> grad_quaternion [N, 4], every row written, culled rows zero (gs_gaussian_normals_backward); rank int32 [N]"""
    N, V = int(quaternion.shape[0]), int(grad_normals.shape[0])
    grad_q = torch.empty(N, 4, dtype=torch.float32, device=quaternion.device)
    _hip.call("gs_gaussian_normals_backward", _p(quaternion), _p(scale), _p(camera_T_world), _p(rank), _p(xyz_cam),
              _p(grad_normals), V, N, _p(grad_q), _stream())
    return grad_q


def depth_normal_forward(depth, alpha, K, min_alpha, raster_mode):
    """-> normal [H, W, 3] of the depth map depth / alpha, zero where invalid (gs_depth_normal)"""
    H, W = int(depth.shape[0]), int(depth.shape[1])
    normal = torch.empty(H, W, 3, dtype=torch.float32, device=depth.device)
    _hip.call("gs_depth_normal", _p(depth), _p(alpha), _p(K), W, H, float(min_alpha), raster_mode, _p(normal), _stream())
    return normal


def depth_normal_backward(depth, alpha, K, grad_normal, min_alpha, raster_mode):
    """-> grad_depth, grad_alpha [H, W], written for every pixel (gs_depth_normal_backward); one allocation"""
    H, W = int(depth.shape[0]), int(depth.shape[1])
    buf = torch.empty(2, H, W, dtype=torch.float32, device=depth.device)
    _hip.call("gs_depth_normal_backward", _p(depth), _p(alpha), _p(K), _p(grad_normal), W, H, float(min_alpha),
              raster_mode, _p(buf[0]), _p(buf[1]), _stream())
    return buf[0], buf[1]


def _as_slab(g_uv, g_conic, g_opa, g_rgb, V, dev):
    """the four render gradients as one [V, 9] slab: the slab they are views of when they come
    straight from _Render.backward, a packed copy otherwise (outputs nobody consumed count as 0)"""
    parts = ((g_rgb, SLAB_RGB), (g_opa, SLAB_OPACITY), (g_uv, SLAB_UV), (g_conic, SLAB_CONIC))
    base = g_rgb._base if g_rgb is not None else None
    if (base is not None and base.dim() == 2 and base.shape[1] == SLAB_WIDTH and base.is_contiguous()
            and all(g is not None and g._base is base and g.shape[0] == V and g.stride() == (SLAB_WIDTH, 1)
                    and g.storage_offset() == base.storage_offset() + sl.start for g, sl in parts)):
        return base
    slab = torch.zeros(max(V, 1), SLAB_WIDTH, dtype=torch.float32, device=dev)
    for g, sl in parts:
        if g is not None:
            slab[:V, sl] = g
    return slab


# ---------------------------------------------------------------------------------------------------
# autograd nodes
# ---------------------------------------------------------------------------------------------------
def _frame_record(width, height, near_thresh, far_thresh, cull_mask_padding, mh_dist, tile_rows=None, sort_prefix=0,
                  background=None, pose_grad=False, adam_plan=None, antialiased=False, z_out=False, may_cut=False,
                  slab_sync=None, absgrad=False, camera_model="pinhole", filter3d=None):
    """What one frame's two nodes share and autograd does not differentiate: the frame's options, set here by the entry
    point, and -- filled by _Preprocess.forward -- the stage record's tensors the render and the caller read.  Handed
    to both nodes as a non-tensor argument.  The differentiable outputs are not kept on it (that would tie the record to
    the graph), and what a backward reads still goes through its ctx.save_for_backward.
    adam_plan: train_ops.FusedRasterAdam's plan -> the per-Gaussian backward steps quaternion, scale, opacity, rgb and
    sh itself (preprocess_backward_adam) and returns a gradient for xyz only
    pose_grad: the frame gives camera_T_world its gradient when it requires one (pose_backward); False keeps the pose a
    constant (multi-GPU frames: the sum would need an all-reduce; per-pixel SH: its rays depend on it)
    z_out (rasterize_rgbd, rasterize_distortion): _Preprocess has one more output, z = xyz_camera_frame[:V, 2] as a differentiable
    tensor -- the handle through which the depth map's dL/dz comes back to that node
    antialiased: the packed record's opacity is sigmoid * comp; the opacity OUTPUT stays the sigmoid (the render reads
    the record), so the gradient that comes back for it is dL/d(sigmoid * comp) and the backward folds it
    camera_model: "pinhole" or "fisheye" -- the projection of the per-Gaussian stage, forward and both backwards; the
    render, the binning and the maps read only what that stage wrote
    filter3d: None, or the float32 [N] variances of the 3D smoothing filter: a constant of the frame that
    the per-Gaussian stage reads forward and backward, carried here next to antialiased
    may_cut: the frame may take the depth cut (want_depth_cut decides); its record, what _Render's two passes need,
    is then left in `cut`
    slab_sync: see rasterize()
    absgrad: rasterize(absgrad=True) -- the entry point leaves a float32 [max(V, 1), 2] buffer in `uv_absgrad` and
    _Render's colour backward fills it (render_backward)"""
    return SimpleNamespace(
        width=width, height=height, near_thresh=near_thresh, far_thresh=far_thresh, cull_mask_padding=cull_mask_padding,
        mh_dist=mh_dist, tile_rows=tile_rows, sort_prefix=sort_prefix, background=background, pose_grad=pose_grad,
        adam_plan=adam_plan, antialiased=bool(antialiased), camera_model=camera_model, filter3d=filter3d, z_out=z_out,
        may_cut=may_cut,
        slab_sync=slab_sync, absgrad=bool(absgrad), uv_absgrad=None,
        # after _Preprocess.forward (xyz_cam and vis_idx: the V visible rows)
        packed=None, xyz_cam=None, culling_mask=None, ranges=None, sorted_g=None, vis_idx=None, rank=None, keys=None,
        cut=None,
        rendered=None)   # (image, nsp, fw, cost, seg) when _Preprocess.forward already enqueued _Render's kernels


class _Preprocess(torch.autograd.Function):
    """parameters, pose, frame record -> uv, conic, opacity, rgb of the visible Gaussians (+ z when fr.z_out);
    everything else the frame made is left on the record"""

    @staticmethod
    def forward(ctx, xyz, quaternion, scale, opacity, rgb, sh, camera_T_world, K, fr):
        ntx, nty = _tile_grid(fr.width, fr.height)
        row0, row1 = fr.tile_rows if fr.tile_rows is not None else (0, nty)
        # (a frame that is rendered from prefix lists always has a background: every entry point passes one)
        cut = (fr.may_cut and fr.sort_prefix != 0 and
               want_depth_cut((xyz.device.index, xyz.shape[0], ntx * nty, row0, row1), xyz.shape[0], ntx, row0, row1,
                              fr.tile_rows is None))
        f = preprocess_forward(xyz, quaternion, scale, opacity, rgb, sh, camera_T_world, K, fr.width, fr.height,
                               fr.near_thresh, fr.far_thresh, fr.cull_mask_padding, fr.mh_dist, fr.tile_rows,
                               fr.sort_prefix, defer=(not cut) and EARLY_RENDER and fr.sort_prefix != 0, depth_cut=cut,
                               antialiased=fr.antialiased, camera_model=fr.camera_model, filter3d=fr.filter3d)
        if cut:
            fr.rendered = render_forward(f.packed, f.rgb_render, f.ranges, f.sorted_g, f.keys, fr.background, fr.height,
                                         fr.width, fr.tile_rows, fr.sort_prefix, segments=False, cut=f.cut)
        elif f.deferred:
            # the render (the _Render node's forward) is enqueued on the speculative tile lists before
            # the host waits for the frame's counts, so a short frame leaves no bubble on the GPU;
            # a too small capacity repeats it
            def render(exact_count):
                seg = segments_for(f.hint_key, f.sorted_buf.shape[0] if not exact_count else f.S, exact_count,
                                   (f.row1 - f.row0) * f.ntx)
                return render_forward(f.packed, f.rgb_render, f.ranges, f.sorted_buf, f.keys_buf, fr.background,
                                      fr.height, fr.width, fr.tile_rows, fr.sort_prefix, segments=seg)

            # (only gs_render_tiles_prefix takes the capacity and skips segments beyond it)
            pre = render(False) if (f.speculative and f.capacity > fr.sort_prefix) else None
            if preprocess_finish(f) or pre is None:
                pre = render(True)
            fr.rendered = pre
        V = f.V
        fr.packed, fr.xyz_cam, fr.culling_mask, fr.ranges = f.packed, f.xyz_cam[:V], f.culling_mask, f.ranges
        fr.sorted_g, fr.vis_idx, fr.rank, fr.keys, fr.cut = f.sorted_g, f.vis_idx[:V], f.rank, f.keys, f.cut
        ctx.save_for_backward(xyz, quaternion, scale, camera_T_world, K)
        ctx.set_materialize_grads(False)   # no zero tensor for an output nobody consumed
        ctx.fr = fr
        ctx.f = SimpleNamespace(N=f.N, V=V, n_sh=f.n_sh, center=f.center, rank=f.rank, opacity_act=f.opacity_act,
                                vis_idx=fr.vis_idx)
        out = (f.uv[:V], f.conic[:V], f.opacity_act[:V], f.rgb_render[:V])
        return out + (f.xyz_cam[:V, 2].contiguous(),) if fr.z_out else out

    @staticmethod
    def backward(ctx, g_uv, g_conic, g_opa, g_rgb, g_z=None):
        xyz, quaternion, scale, camera_T_world, K = ctx.saved_tensors
        fr = ctx.fr
        slab = _as_slab(g_uv, g_conic, g_opa, g_rgb, ctx.f.V, xyz.device)
        g_z = g_z.contiguous() if (g_z is not None and ctx.f.V > 0) else None
        if _keep_slab:
            global _last_grad_z
            _note_slab(slab, ctx.f.V)
            _last_grad_z = g_z
        # (before the fused optimizer step, which overwrites the quaternion and scale the pose terms read)
        g_pose = None
        if fr.pose_grad and ctx.needs_input_grad[6]:
            g_pose = pose_backward(xyz, quaternion, scale, camera_T_world, K, ctx.f, slab, antialiased=fr.antialiased,
                                   camera_model=fr.camera_model, filter3d=fr.filter3d)
            if g_z is not None:
                # the direct term of z = T[2, 0:3] . xyz + T[2, 3] (the slab's terms above already hold the depth map's
                # uv / conic columns): plumbing on the visible rows, not a hot path
                gz64 = g_z.double()   # (float64 sums: V terms of mixed sign)
                g_pose[2, :3] += (gz64 @ xyz.index_select(0, ctx.f.vis_idx.long()).double()).float()
                g_pose[2, 3] += gz64.sum().float()
        if fr.adam_plan is not None:
            grads = (preprocess_backward_adam(xyz, camera_T_world, K, ctx.f, slab, fr.adam_plan),) + (None,) * 5
        else:
            grads = preprocess_backward(xyz, quaternion, scale, camera_T_world, K, ctx.f, slab,
                                        antialiased=fr.antialiased, camera_model=fr.camera_model, filter3d=fr.filter3d)
        if g_z is not None:
            _hip.call("gs_z_backward", _p(ctx.f.rank), _p(g_z), _p(camera_T_world), 0, ctx.f.N, _p(grads[0]), _stream())
        return grads + (g_pose, None, None)   # (K, the record)


class _DepthMap:
    """_Render's map policy of rasterize_rgbd (DepthFwd / DepthBwd of csrc/render.hip): channel z [V] -> depth, alpha
    [H, W] (gs_render_zalpha / gs_render_zalpha_backward); dL/dz is a tail behind the slab's rows, cleared with them"""
    forward, backward = staticmethod(zalpha_forward), staticmethod(zalpha_backward)
    extra = False   # no fourth output
    # what the kernels read: the record's camera-frame positions; z is only the handle dL/dz goes back through
    source = staticmethod(lambda fr, z: fr.xyz_cam)
    tail = staticmethod(lambda V: max(V, 1))   # floats behind the slab's rows

    @staticmethod
    def channel_grad(xyz_cam, V, tail, grad_depth, wanted):
        """-> (what the backward kernel adds dL/dz to, the gradient of z)"""
        return tail, (tail[:V] if grad_depth is not None else None)   # (alpha alone leaves dL/dz None)


class _DistortionMap(_DepthMap):
    """_Render's map policy of rasterize_distortion (DistortionFwd, k_render_distortion_bwd): _DepthMap with one more
    output, the depth distortion [H, W], from gs_render_distortion / gs_render_distortion_backward IN PLACE of the depth
    kernels; the backward reads the forward's depth and alpha, and dL/dz (from depth's or distortion's gradient) takes
    _DepthMap's way"""
    forward, backward = staticmethod(distortion_forward), staticmethod(distortion_backward)
    extra = True    # forward -> ((depth, distortion), alpha, T_end); backward(..., t_end, depth, alpha, g_dist, g_depth, ...)
    keep = staticmethod(lambda depth, alpha, distortion: (depth, alpha))   # the totals its backward reads


class _MedianDepthMap(_DepthMap):
    """_Render's map policy of rasterize_median_depth (MedianFwd, k_median_depth_bwd): _DepthMap with two more outputs,
    median_depth (differentiable in z alone) and median_index (int32, marked non-differentiable), from
    gs_render_median_depth IN PLACE of gs_render_zalpha.  The backward is two independent launches into the same slab
    and dL/dz tail: gs_render_zalpha_backward if depth or alpha has a gradient, gs_median_depth_backward if
    median_depth has one"""
    forward = staticmethod(median_depth_forward)
    extra = True    # forward -> ((depth, median_depth, median_index), alpha, T_end)
    keep = staticmethod(lambda depth, alpha, median_depth, median_index: (median_index,))

    @staticmethod
    def backward(packed, xyz_cam, ranges, sorted_g, nsp, t_end, median_index, grad_median, grad_index, grad_depth,
                 grad_alpha, height, width, slab, grad_z):
        if grad_depth is not None or grad_alpha is not None:
            zalpha_backward(packed, xyz_cam, ranges, sorted_g, nsp, t_end, grad_depth, grad_alpha, height, width, slab,
                            grad_z)
        if grad_median is not None:
            median_depth_backward(median_index, grad_median, height, width, grad_z)


class _FeatureMap:
    """_Render's map policy of rasterize_features (FeaturesFwd / FeaturesBwd): channels feat [V, C], the visible
    Gaussians' rows -> feature_map [H, W, C], alpha [H, W] (gs_render_features / gs_render_features_backward)"""
    forward, backward = staticmethod(features_forward), staticmethod(features_backward)
    extra = False
    source = staticmethod(lambda fr, feat: feat)
    tail = staticmethod(lambda V: 0)

    @staticmethod
    def channel_grad(feat, V, tail, grad_map, wanted):
        """-> (grad_features for the backward kernel, the gradient of feat): NULL unless feat requires a gradient and
        feature_map has one"""
        g_feat = torch.zeros_like(feat) if (grad_map is not None and wanted) else None
        return g_feat, g_feat


class _Render(torch.autograd.Function):
    """uv, conic, opacity, rgb, the map policy's channels (None without one), the frame record, the policy -> image,
    or (image, map, alpha) with a policy (+ its extra maps when it declares some): its kernels run on the lists and the
    splat counts the colour forward left.
    One backward for all outputs: the prologue clears the slab (and the policy's tail), the colour backward runs if
    the image has a gradient, the policy's if its map or alpha has one, and _Preprocess gets the one slab plus the
    channels' gradient.  An unused output costs no launch."""

    @staticmethod
    def forward(ctx, uv, conic, opacity, rgb, channels, fr, policy):
        rendered, fr.rendered = fr.rendered, None
        image, nsp, fw, cost, seg = rendered if rendered else render_forward(
            fr.packed, rgb, fr.ranges, fr.sorted_g, fr.keys, fr.background, fr.height, fr.width, fr.tile_rows,
            fr.sort_prefix)
        saved = (fr.packed, rgb, fr.ranges, fr.sorted_g, fr.background, nsp, fw, cost, seg)
        out = image
        if policy is not None:
            source = policy.source(fr, channels)
            fmap, alpha, t_end = policy.forward(fr.packed, source, fr.ranges, fr.sorted_g, nsp, fr.height, fr.width)
            saved += (source, t_end)
            out = (image, fmap, alpha)
            if policy.extra:   # (map, extra maps...): further outputs, and a backward that reads what keep() names
                fmap, *extras = fmap
                saved += policy.keep(fmap, alpha, *extras)
                ctx.mark_non_differentiable(*(e for e in extras if not e.is_floating_point()))
                out = (image, fmap, alpha, *extras)
        ctx.save_for_backward(*saved)
        ctx.set_materialize_grads(False)
        ctx.fr, ctx.policy, ctx.V = fr, policy, uv.shape[0]   # (fr.cut: flags, complete ranges, overflow lists)
        # the gradient mode of THIS frame is the default at its forward: a later set_backward_mode() cannot
        # race the backward the autograd engine runs on its own thread
        ctx.backward_mode = _hip.get_backward_mode()
        return out

    @staticmethod
    def backward(ctx, grad_image, grad_map=None, grad_alpha=None, *grad_extra):
        packed, rgb, ranges, sorted_g, background_rgb, nsp, fw, cost, seg, *mapped = ctx.saved_tensors
        fr, policy, V = ctx.fr, ctx.policy, ctx.V
        if grad_image is None and grad_map is None and grad_alpha is None and all(g is None for g in grad_extra):
            return (None,) * len(ctx.needs_input_grad)
        n_tail = policy.tail(V) if policy is not None else 0
        out = render_backward(packed, rgb, ranges, sorted_g, background_rgb, nsp, fw,
                              grad_image.contiguous() if grad_image is not None else None, fr.height, fr.width,
                              fr.tile_rows, V, cost, ctx.backward_mode, seg, cut=fr.cut, tail=n_tail,
                              uv_absgrad=fr.uv_absgrad)
        slab, tail = out if n_tail else (out, None)
        g_channels = None
        if policy is not None:
            source, t_end, *totals = mapped   # (totals: what the policy's keep() named of the forward's outputs)
            maps = (*grad_extra, grad_map) if policy.extra else (grad_map,)
            into, g_channels = policy.channel_grad(source, V, tail, next((m for m in maps if m is not None), None),
                                                   ctx.needs_input_grad[4])
            # (nothing visible: nothing to add, and an empty slab has no address)
            if (any(m is not None for m in maps) or grad_alpha is not None) and V > 0:
                policy.backward(packed, source, ranges, sorted_g, nsp, t_end, *totals, *maps, grad_alpha, fr.height,
                                fr.width, slab, into)
        if fr.slab_sync is not None:
            fr.slab_sync(slab.view(-1))   # multi-GPU: sum the partial gradients of all bands in place
        # the four gradients are views of the one slab; _Preprocess.backward recognises that
        return slab[:, SLAB_UV], slab[:, SLAB_CONIC], slab[:, SLAB_OPACITY], slab[:, SLAB_RGB], g_channels, None, None


class _GatherRows(torch.autograd.Function):
    """rows `index` (unique, int64) of a dense parameter tensor; the gradient is an index_copy into zeros
    (torch's own indexing backward sorts the indices to accumulate duplicates: there are none)"""

    @staticmethod
    def forward(ctx, dense, index):
        ctx.save_for_backward(index)
        ctx.shape = dense.shape
        return dense.index_select(0, index)

    @staticmethod
    def backward(ctx, grad):
        (index,) = ctx.saved_tensors
        return torch.zeros(ctx.shape, dtype=grad.dtype, device=grad.device).index_copy_(0, index, grad), None


class _GaussianNormals(torch.autograd.Function):
    """quaternion, scale, pose, the frame record (after _Preprocess.forward) -> normals [V, 3] of the visible Gaussians.
    The axis choice and the flip are constants: scale gets no gradient, and neither does xyz (the record's xyz_cam is read
    for the flip's sign only).  The pose's direct term, n_c = W n_w, is plumbing on the visible rows like the z term of
    _Preprocess.backward: dL/dW = sum_v g_v (x) (+-n_w,v), and with W a rotation +-n_w,v = W^T n_c,v, the rows of
    normals @ W; the sum is taken in float64."""

    @staticmethod
    def forward(ctx, quaternion, scale, camera_T_world, fr):
        normals = gaussian_normals_forward(quaternion, scale, camera_T_world, fr.vis_idx, fr.xyz_cam)
        ctx.save_for_backward(quaternion, scale, camera_T_world, normals)
        ctx.fr = fr
        return normals

    @staticmethod
    def backward(ctx, grad):
        quaternion, scale, camera_T_world, normals = ctx.saved_tensors
        fr = ctx.fr
        grad = grad.contiguous()
        if _keep_slab:
            global _last_grad_normals
            _last_grad_normals = grad
        g_q = gaussian_normals_backward(quaternion, scale, camera_T_world, fr.rank, fr.xyz_cam, grad) \
            if ctx.needs_input_grad[0] else None
        g_pose = None
        if ctx.needs_input_grad[2]:
            g_pose = torch.zeros_like(camera_T_world)
            if grad.shape[0] > 0:
                g_pose[:3, :3] = (grad.double().t() @ (normals.double() @ camera_T_world[:3, :3].double())).float()
        return g_q, None, g_pose, None


class _DepthNormal(torch.autograd.Function):
    """depth, alpha [H, W], K -> the depth map's normal [H, W, 3]; the validity decisions are constants"""

    @staticmethod
    def forward(ctx, depth, alpha, K, min_alpha, raster_mode):
        ctx.save_for_backward(depth, alpha, K)
        ctx.options = (min_alpha, raster_mode)
        return depth_normal_forward(depth, alpha, K, min_alpha, raster_mode)

    @staticmethod
    def backward(ctx, grad):
        depth, alpha, K = ctx.saved_tensors
        g_depth, g_alpha = depth_normal_backward(depth, alpha, K, grad.contiguous(), *ctx.options)
        return g_depth, g_alpha, None, None, None


class _RenderSH(torch.autograd.Function):
    """Per-pixel SH colour (rasterize.py:100-110 with use_sh_precompute=False; render.cu:283-333,
    render_backward.cu:422-488): the N_SH in {4, 9, 16} render kernels on the fused frame's packed records and
    tile lists.  coeffs: [V, 3, N_SH] colour coefficients of the visible Gaussians, rays: [H, W, 3]."""

    @staticmethod
    def forward(ctx, uv, conic, opacity, coeffs, packed, ranges, sorted_g, rays, background_rgb, height, width,
                tile_rows):
        dev = packed.device
        nty = _tile_grid(width, height)[1]
        row0, row1 = tile_rows if tile_rows is not None else (0, nty)
        alloc = torch.empty if tile_rows is None else torch.zeros
        P = height * width
        buf = alloc(5 * P, dtype=torch.float32, device=dev)
        image, fw = buf[:3 * P].view(height, width, 3), buf[3 * P:4 * P].view(height, width)
        nsp = buf[4 * P:].view(torch.int32).view(height, width)
        _hip.call("gs_render_tiles_packed", _p(packed), _p(coeffs), _p(rays), _p(ranges), _p(sorted_g),
                  _p(background_rgb), width, height, int(coeffs.shape[2]), row0, row1, _p(nsp), _p(fw), _p(image),
                  _hip.GS_F32, None, _stream())
        ctx.save_for_backward(packed, coeffs, ranges, sorted_g, rays, background_rgb, nsp, fw)
        ctx.set_materialize_grads(False)
        ctx.dims = (height, width, row0, row1, uv.shape[0])
        ctx.backward_mode = _hip.get_backward_mode()   # the frame's mode is the default at its forward
        return image

    @staticmethod
    def backward(ctx, grad_image):
        packed, coeffs, ranges, sorted_g, rays, background_rgb, nsp, fw = ctx.saved_tensors
        height, width, row0, row1, V = ctx.dims
        if grad_image is None:
            return (None,) * 12
        n_sh = int(coeffs.shape[2])
        (gc, go, gu, gk) = _Arena(torch.float32, packed.device, (3 * n_sh * V, V, 2 * V, 3 * V), zero=True).blocks()
        g_rgb, g_opa, g_uv, g_conic = gc.view(V, 3, n_sh), go.view(V, 1), gu.view(V, 2), gk.view(V, 3)
        _hip.call("gs_render_tiles_backward_packed", _p(packed), _p(coeffs), _p(rays), _p(ranges), _p(sorted_g),
                  _p(background_rgb), _p(nsp), _p(fw), _p(grad_image.contiguous()), width, height, n_sh, row0, row1,
                  _p(g_rgb), _p(g_opa), _p(g_uv), _p(g_conic), _hip.GS_F32, int(ctx.backward_mode), _stream())
        return (g_uv, g_conic, g_opa, g_rgb) + (None,) * 8


def _rasterize_per_pixel_sh(g, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                            background_rgb, tile_rows):
    """use_sh_precompute=False on the fused frame: its per-Gaussian stage, binning and full per-tile sort, the
    colour coefficients of the visible Gaussians gathered once, and the per-pixel-SH render kernels.  Same
    (image, culling_mask, uv) contract and the same kernels as the reference-shaped path of this colour mode
    (which spends ~4 ms per frame of workload B in its host glue); against it the frame differs as the
    precompute mode's does: by the fused per-Gaussian stage's explicit fp32 world->camera transform."""
    # (sh=None: the per-Gaussian stage computes no colour; full sort, no early render; the rays depend on the pose)
    fr, (uv, conic, opacity, _rgb_unused) = _begin_frame(
        g, None, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist, background_rgb,
        tile_rows=tile_rows)
    index = fr.vis_idx.long()
    # coefficient 0 is the rgb parameter (rasterize.py:103: cat of rgb and sh)
    coeffs = torch.cat((_GatherRows.apply(g.rgb, index).unsqueeze(2), _GatherRows.apply(g.sh, index)), dim=2)
    rays = compute_rays_in_world_frame(camera, camera_T_world)
    image = _RenderSH.apply(uv, conic, opacity, coeffs.contiguous(), fr.packed, fr.ranges, fr.sorted_g, rays,
                            fr.background, fr.height, fr.width, tile_rows)
    return image, fr.culling_mask, uv


def render_depth(gaussians, alpha_threshold, camera_T_world, camera, near_thresh, cull_mask_padding, mh_dist):
    """splat_py.depth.render_depth (depth.py:17-88) on the fused frame's stages: [H, W, 1], the distance of the
    first Gaussian at which a pixel's accumulated alpha passes alpha_threshold, -1 where it never does.  No
    gradient.  The reference's depth path has no far threshold (depth.py:33-41): none is applied."""
    g = gaussians
    if not g.xyz.is_cuda or g.xyz.dtype != torch.float32:
        from .splat_py.depth import render_depth as reference_shaped
        return reference_shaped(g, alpha_threshold, camera_T_world, camera, near_thresh, cull_mask_padding, mh_dist)
    with torch.no_grad():
        W, H = int(camera.width), int(camera.height)
        f = preprocess_forward(g.xyz.contiguous(), g.quaternion.contiguous(), g.scale.contiguous(),
                               g.opacity.contiguous(), g.rgb.contiguous(), None, camera_T_world.contiguous(),
                               camera.K.contiguous(), W, H, near_thresh, 3.0e38, cull_mask_padding, mh_dist, None, 0)
        depth = torch.full((H, W, 1), -1.0, dtype=torch.float32, device=g.xyz.device)
        _hip.call("gs_render_depth", _p(f.packed), _p(f.xyz_cam), _p(f.ranges), _p(f.sorted_g), W, H,
                  alpha_threshold, _p(depth), _stream())
        return depth


def _require(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def validate(gaussians, camera_T_world, camera, background_rgb, filter3d=None):
    """The checks of the reference's extension (src/checks.cuh:5-14, render.cu:204-246) for the tensors the
    fused path hands to the C ABI as raw pointers: device, dtype, shape.  (Contiguity is established by
    the caller with .contiguous().)  Raises RuntimeError like the reference's TORCH_CHECKs."""
    g = gaussians
    dev = g.xyz.device
    N = g.xyz.shape[0]
    named = (("xyz", g.xyz, (N, 3)), ("quaternion", g.quaternion, (N, 4)), ("scale", g.scale, (N, 3)),
             ("opacity", g.opacity, (N, 1)), ("rgb", g.rgb, (N, 3)), ("camera_T_world", camera_T_world, (4, 4)),
             ("K", camera.K, (3, 3)), ("background_rgb", background_rgb, (3,)))
    for name, t, shape in named:
        _require(t.is_cuda and t.device == dev, f"{name} is not a CUDA tensor on {dev}")
        _require(t.dtype == torch.float32, f"{name} is not a float tensor")
        _require(tuple(t.shape) == shape, f"{name} must have shape {list(shape)}, got {list(t.shape)}")
    if g.sh is not None:
        t = g.sh
        _require(t.is_cuda and t.device == dev, f"sh is not a CUDA tensor on {dev}")
        _require(t.dtype == torch.float32, "sh is not a float tensor")
        _require(t.dim() == 3 and t.shape[0] == N and t.shape[1] == 3 and t.shape[2] in (3, 8, 15),
                 f"sh must have shape [{N}, 3, 3|8|15], got {list(t.shape)}")
    if filter3d is not None:
        t = filter3d
        _require(torch.is_tensor(t) and t.is_cuda and t.device == dev, f"filter3d is not a CUDA tensor on {dev}")
        _require(t.dtype == torch.float32, "filter3d is not a float tensor")
        _require(tuple(t.shape) == (N,), f"filter3d must have shape [{N}], one variance per Gaussian, got {list(t.shape)} "
                                         "(recompute the filter after a step that changes N)")


def supported(gaussians, camera_T_world, camera, use_sh_precompute):
    if not gaussians.xyz.is_cuda or gaussians.xyz.dtype != torch.float32:
        return False
    if gaussians.sh is not None and not use_sh_precompute:
        return False   # per-pixel SH evaluation: not the two-node frame (rasterize() routes it, see there)
    return True


def _refuse(who, gaussians, camera_T_world, camera, use_sh_precompute, background_rgb, frame_options, adam_plan,
            filter3d=None):
    """what the antialiased frame and the map frames (`who`) are served on, checked before anything is enqueued: each
    refusal names its reason.  filter3d: the frame's 3D smoothing filter, if it has one -- float32 [N] on the Gaussians'
    device, a constant (no requires_grad)"""
    g = gaussians
    _require(not any(frame_options),
             f"{who} serves whole single-GPU frames: tile_rows, return_aux, grad_sync, slab_sync and "
             "frame_hook are not supported")
    _require(adam_plan is None, f"{who} does not take the fused optimizer step (adam_plan)")
    _require(g.sh is None or use_sh_precompute,
             f"{who} needs the SH-precompute colour mode: per-pixel SH (use_sh_precompute=False) is not supported")
    tensors = [t for t in (g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, camera_T_world, camera.K,
                           background_rgb) if t is not None]
    _require(all(t.is_cuda and t.dtype == torch.float32 for t in tensors),
             f"{who} needs float32 tensors on the GPU (no fp64, no CPU path)")
    if filter3d is not None:
        _require(torch.is_tensor(filter3d) and filter3d.dtype == torch.float32 and filter3d.device == g.xyz.device
                 and tuple(filter3d.shape) == (g.xyz.shape[0],),
                 f"{who}: filter3d must be float32 [N] on the Gaussians' device, one variance per Gaussian "
                 "(recompute the filter after a step that changes N)")
        _require(not filter3d.requires_grad, f"{who}: filter3d is a constant of the frame and must not require a gradient")


def _begin_frame(gaussians, sh, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                 background_rgb, who=None, use_sh_precompute=True, frame_options=(), features=None, adam_plan=None,
                 **options):
    """What every entry point does before its render node.  who (rasterize_rgbd, rasterize_features,
    rasterize_contributions): refuse what that frame kind does not serve and validate; None: rasterize() has done both
    before it chose this orchestration.  Then make the inputs contiguous and run _Preprocess on a frame record with
    `options` (_frame_record's; a `who` frame sorts as SORT_PREFIX says and gives the pose its gradient; without
    may_cut the depth cut stays off -- a cut frame's flagged tiles keep their lists elsewhere).  `sh`: the
    coefficients the per-Gaussian stage folds into the colour.
    -> (the frame record, (uv, conic, opacity, rgb[, z]))"""
    g = gaussians
    _raster_mode(False, options.get("camera_model", "pinhole"))   # (an unknown name raises before anything else)
    filter3d = options.get("filter3d")
    if who is not None:
        _refuse(who, g, camera_T_world, camera, use_sh_precompute, background_rgb, frame_options, adam_plan, filter3d)
        if features is not None:
            _require(torch.is_tensor(features) and features.dim() == 2 and features.shape[0] == g.xyz.shape[0],
                     f"{who}: features must be [N, C], one row per Gaussian")
            _require(1 <= features.shape[1] <= 32,
                     f"{who}: features must have 1 to 32 columns (callers with more split the channels)")
            _require(features.dtype == torch.float32 and features.device == g.xyz.device,
                     f"{who}: features must be float32 on the Gaussians' device (no fp64, no CPU path)")
        validate(g, camera_T_world, camera, background_rgb, filter3d)
        options = dict(options, sort_prefix=_hip.GS_SORT_PREFIX if SORT_PREFIX else 0, pose_grad=True)
    if filter3d is not None:
        options = dict(options, filter3d=filter3d.contiguous())
    fr = _frame_record(int(camera.width), int(camera.height), near_thresh, far_thresh, cull_mask_padding, mh_dist,
                       background=background_rgb.contiguous(), adam_plan=adam_plan, **options)
    return fr, _Preprocess.apply(
        g.xyz.contiguous(), g.quaternion.contiguous(), g.scale.contiguous(), g.opacity.contiguous(), g.rgb.contiguous(),
        sh.contiguous() if sh is not None else None, camera_T_world.contiguous(), camera.K.contiguous(), fr)


def rasterize(gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
              use_sh_precompute, background_rgb, tile_rows=None, return_aux=False, grad_sync=None, slab_sync=None,
              frame_hook=None, adam_plan=None, antialiased=False, absgrad=False, camera_model="pinhole", filter3d=None):
    """tile_rows=(row0, row1) restricts binning and rendering to those tile rows; slab_sync(flat) is
    called on the flat [9 V] render-gradient slab in the backward (grad_sync is the generic
    per-tensor form used by the reference-shaped path): the hooks gaussian_splatting_amd.sharded
    uses; all default to the single-GPU behaviour.  frame_hook(dict) receives the frame's tile ranges.
    adam_plan: only train_ops.FusedRasterAdam.rasterize passes it (the per-Gaussian backward then steps
    quaternion, scale, opacity, rgb and sh itself): whole single-GPU frames without hooks, SH-precompute colour.
    antialiased=True multiplies every splat's opacity by sqrt(det Sigma_2D / det(Sigma_2D + 0.25 I)), so that the 0.25 px^2
    dilation of the fp32 record no longer adds light to splats smaller than a pixel, and differentiates through the
    factor: whole single-GPU fp32 frames without hooks or adam_plan in the SH-precompute colour mode,
    anything else raises RuntimeError before a kernel is enqueued.
    absgrad=True (AbsGS, gsplat's absgrad) returns a fourth value,

        image, culling_mask, uv, uv_absgrad = rasterize(..., absgrad=True)

    with image, culling_mask and uv those of the plain call, bit for bit.  uv_absgrad is float32 [V, 2] without a
    gradient: zero until the image's backward has run, then for every visible Gaussian the sum over pixels and list
    entries of |dL/du|, |dL/dv| of that pixel's visit -- the magnitudes of the very terms whose signed sum is uv.grad --
    of the MOST RECENT backward (a second backward over a retained graph overwrites).  Hand it to
    densify.DensityController.accumulate in place of uv.grad: per-pixel gradients of opposite sign cancel in uv.grad
    for exactly the large Gaussians that need splitting, and add here.  Served like antialiased=True (which combines
    freely), on the Python orchestration -- the native frame has no such node -- with the depth cut, depth segments and
    longest-first order under their usual policies; anything else raises RuntimeError before a kernel is enqueued.
    camera_model="fisheye" projects with the equidistant fisheye model (gsplat's camera_model="fisheye"):
    uv = (fx, fy) * theta / r * (x, y) + (cx, cy) with theta = atan2(r, z), r = |(x, y)| of the camera-frame position;
    camera.K stays the 3x3 pinhole matrix (no skew, no distortion coefficients) and the cull keeps its form, so the field
    of view stays under 180 degrees.  Only the per-Gaussian stage changes, forward and backward (pose included).  Served
    like antialiased=True, with which and with absgrad=True it combines, natively or on the Python orchestration, with
    the depth cut, depth segments and longest-first order under their usual policies; tile_rows, the hooks, adam_plan,
    per-pixel SH (its rays are pinhole rays), non-fp32 or CPU tensors raise RuntimeError before a kernel is enqueued,
    and so does any other camera_model string.  "pinhole" (the default) is exactly the frame without the keyword.
    filter3d: float32 [N] on the Gaussians' device, the world-space variances phi >= 0 of Mip-Splatting's 3D smoothing
    filter (filter3d_rate and filter3d_from_rate make them from the training cameras).  Every Gaussian is
    rendered with Sigma + phi I and with its opacity times sqrt(prod_k s_k^2 / (s_k^2 + phi)), and the factor is
    differentiated towards scale and opacity; the filter itself is a constant (a tensor that requires a gradient is
    refused) and has to be recomputed after any step that changes N.  Served like antialiased=True -- its other half --
    with which, with absgrad and with camera_model it combines, natively or on the Python orchestration; refused by name
    where that is.  None (the default) is exactly the frame without the keyword; a row with phi = 0 carries that frame's
    values."""
    hooks = return_aux or grad_sync or slab_sync or frame_hook
    raster_mode = _raster_mode(antialiased, camera_model)
    # the options that are served on whole single-GPU fp32 frames only: one refusal, named after those in use
    options = [name for name, on in (("filter3d=", filter3d is not None), ('camera_model="fisheye"', camera_model == "fisheye"),
                                     ("absgrad=True", absgrad), ("antialiased=True", antialiased)) if on]
    if options:
        _refuse(f"rasterize({', '.join(options)})", gaussians, camera_T_world, camera, use_sh_precompute, background_rgb,
                (tile_rows is not None, hooks), adam_plan, filter3d)
    if adam_plan is not None:
        _require(not hooks and tile_rows is None, "the fused optimizer step serves whole single-GPU frames without hooks")
        _require(supported(gaussians, camera_T_world, camera, use_sh_precompute),
                 "the fused optimizer step needs fp32 device tensors and the SH-precompute colour mode")
    if (gaussians.sh is not None and not use_sh_precompute and not hooks and gaussians.xyz.is_cuda
            and gaussians.xyz.dtype == torch.float32):
        # per-pixel SH evaluation (N_SH in {4, 9, 16} render kernels) on the fused frame's stages: single-GPU frames;
        # the multi-GPU hooks of this colour mode stay on the reference-shaped path
        validate(gaussians, camera_T_world, camera, background_rgb)
        return _rasterize_per_pixel_sh(gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding,
                                       mh_dist, background_rgb, tile_rows)
    if not supported(gaussians, camera_T_world, camera, use_sh_precompute):
        return _reference_shaped.rasterize(gaussians, camera_T_world, camera, near_thresh, far_thresh,
                                           cull_mask_padding, mh_dist, use_sh_precompute, background_rgb,
                                           tile_rows=tile_rows, grad_sync=grad_sync)
    g = gaussians
    validate(g, camera_T_world, camera, background_rgb, filter3d)
    nat = native() if not (hooks or absgrad) else None
    if nat is not None:
        nat.set_modes(bool(SORT_PREFIX), bool(EARLY_RENDER))
        nat.set_segments(0 if SEGMENTS == "auto" else (1 if SEGMENTS else -1))
        nat.set_depth_cut(0 if DEPTH_CUT == "auto" else (1 if DEPTH_CUT else -1), int(DEPTH_CUT_MIN_MEAN_LIST))
        row0, row1 = tile_rows if tile_rows is not None else (0, -1)
        if adam_plan is not None:
            return nat.rasterize_adam(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, camera_T_world, camera.K,
                                      int(camera.width), int(camera.height), near_thresh, far_thresh, cull_mask_padding,
                                      mh_dist, background_rgb, adam_plan)
        return nat.rasterize(g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, camera_T_world, camera.K,
                             int(camera.width), int(camera.height), near_thresh, far_thresh, cull_mask_padding, mh_dist,
                             background_rgb, row0, row1, raster_mode, filter3d)
    # (refused and validated above; the depth cut only without hooks; the pose a constant on multi-GPU frames)
    fr, (uv, conic, opacity, rgb) = _begin_frame(
        g, g.sh, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist, background_rgb,
        adam_plan=adam_plan, tile_rows=tile_rows, sort_prefix=_hip.GS_SORT_PREFIX if (SORT_PREFIX and not return_aux) else 0,
        pose_grad=not (grad_sync or slab_sync), antialiased=antialiased, may_cut=not hooks, slab_sync=slab_sync,
        absgrad=absgrad, camera_model=camera_model, filter3d=filter3d)
    if absgrad:   # (a row even when nothing is visible: an empty tensor has no address to hand to the entry)
        fr.uv_absgrad = torch.zeros(max(uv.shape[0], 1), 2, dtype=torch.float32, device=uv.device)
    if frame_hook is not None:   # multi-GPU cost-balanced bands: the band's tile ranges
        frame_hook(dict(ranges=fr.ranges, ntx=_tile_grid(fr.width, fr.height)[0]))
    image = _Render.apply(uv, conic, opacity, rgb, None, fr, None)
    if return_aux:
        return image, fr.culling_mask, uv, dict(conic=conic, opacity=opacity, rgb=rgb, packed=fr.packed,
                                                xyz_camera_frame=fr.xyz_cam, tile_ranges=fr.ranges,
                                                sorted_gaussians=fr.sorted_g, vis_idx=fr.vis_idx)
    if absgrad:
        return image, fr.culling_mask, uv, fr.uv_absgrad[:uv.shape[0]]
    return image, fr.culling_mask, uv


def rasterize_rgbd(gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                   use_sh_precompute, background_rgb, tile_rows=None, return_aux=False, grad_sync=None, slab_sync=None,
                   frame_hook=None, adam_plan=None, antialiased=False, camera_model="pinhole", filter3d=None):
    """rasterize() with a differentiable depth map and accumulated opacity:

        image, depth, alpha, culling_mask, uv = rasterize_rgbd(...)

    image, culling_mask and uv are those of rasterize() on the same inputs, bit for bit.  depth [H, W] = sum_k w_k z_k
    with z the camera-frame z of the Gaussian and w_k = alpha_k T_k the compositing weights of the entries the colour
    forward walked; alpha [H, W] = sum_k w_k.  No background term, depth is not normalised (callers form
    depth / alpha).  All three carry gradients to the Gaussians' parameters and, when it requires one, to
    camera_T_world; the backward of depth and alpha is their true derivative (DESIGN.md "Depth and alpha maps").
    Whole single-GPU fp32 frames in the SH-precompute colour mode, Python orchestration, depth cut off: anything
    else raises RuntimeError (the trailing keyword arguments exist only to say so).  antialiased: as rasterize()'s --
    the maps' weights then carry the antialiased opacity too.  camera_model: as rasterize()'s; depth stays the camera-frame
    z, not the distance along the ray.  filter3d: as rasterize()'s."""
    fr, (uv, conic, opacity, rgb, z) = _begin_frame(
        gaussians, gaussians.sh, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
        background_rgb, "rasterize_rgbd", use_sh_precompute,
        (tile_rows is not None, return_aux, grad_sync, slab_sync, frame_hook), adam_plan=adam_plan,
        antialiased=antialiased, z_out=True, camera_model=camera_model, filter3d=filter3d)
    image, depth, alpha = _Render.apply(uv, conic, opacity, rgb, z, fr, _DepthMap)
    return image, depth, alpha, fr.culling_mask, uv


def rasterize_distortion(gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                         use_sh_precompute, background_rgb, tile_rows=None, return_aux=False, grad_sync=None,
                         slab_sync=None, frame_hook=None, adam_plan=None, antialiased=False,
                         camera_model="pinhole", filter3d=None):
    """rasterize_rgbd() with the depth-distortion map of the same walk:

        image, depth, alpha, distortion, culling_mask, uv = rasterize_distortion(...)

    image, culling_mask and uv are those of rasterize(), depth and alpha those of rasterize_rgbd() on the same inputs,
    bit for bit.  distortion [H, W] = 2 sum_k w_k (z_k A_<k - D_<k) with A_<k, D_<k the sums of w_j and w_j z_j over
    the contributors in front of entry k: on the frame's lists, which are sorted by z, sum_{i,j} w_i w_j |z_i - z_j|,
    the distortion loss of Mip-NeRF 360 / 2DGS.  No background term, no normalisation by alpha, no depth warp: the
    value is in units of z (callers scale z, or divide by alpha^2).  All four outputs carry gradients to the Gaussians'
    parameters and, when it requires one, to camera_T_world; the maps' backward is their true derivative, one kernel
    for the three of them in place of rasterize_rgbd's (DESIGN.md "Depth distortion").  An output without a gradient
    costs nothing.  Whole single-GPU fp32 frames in the SH-precompute colour mode, Python orchestration, depth cut off:
    anything else raises RuntimeError (the trailing keyword arguments exist only to say so).  antialiased, camera_model,
    filter3d: as rasterize()'s."""
    fr, (uv, conic, opacity, rgb, z) = _begin_frame(
        gaussians, gaussians.sh, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
        background_rgb, "rasterize_distortion", use_sh_precompute,
        (tile_rows is not None, return_aux, grad_sync, slab_sync, frame_hook), adam_plan=adam_plan,
        antialiased=antialiased, z_out=True, camera_model=camera_model, filter3d=filter3d)
    image, depth, alpha, distortion = _Render.apply(uv, conic, opacity, rgb, z, fr, _DistortionMap)
    return image, depth, alpha, distortion, fr.culling_mask, uv


def rasterize_median_depth(gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                           use_sh_precompute, background_rgb, tile_rows=None, return_aux=False, grad_sync=None,
                           slab_sync=None, frame_hook=None, adam_plan=None, antialiased=False,
                           camera_model="pinhole", filter3d=None):
    """rasterize_rgbd() with the median depth of the same walk (2DGS's depth_ratio = 1, gsplat's median depth):

        image, depth, alpha, median_depth, median_index, culling_mask, uv = rasterize_median_depth(...)

    image, culling_mask and uv are those of rasterize(), depth and alpha those of rasterize_rgbd() on the same inputs,
    bit for bit.  The median entry of a pixel is the last contributing list entry in front of which the transmittance
    is still above 0.5: the entry during which T falls to 0.5 or below, or the last contributor where it never falls
    that far (2DGS's `if (T > 0.5) median = depth`).  median_depth [H, W] is the camera-frame z of that
    entry's Gaussian -- not weighted, not normalised, always a splat's own z where the expected depth / alpha lies
    between the surfaces at a semi-transparent edge -- and 0 where the pixel has no contributor.  median_index [H, W]
    int32 is that Gaussian's row in the caller's dense numbering, -1 where the pixel has no contributor; it carries no
    gradient.  A caller who wants only the pixels whose transmittance did cross 0.5 masks with alpha >= 0.5; the valid
    pixels are median_index >= 0.  median_depth is differentiated with the choice of entry held constant: its
    gradient reaches xyz (and camera_T_world when it requires one) through z alone, nothing goes to uv, conic or
    opacity.  image, depth and alpha keep rasterize_rgbd's gradients; an output without a gradient costs no launch.
    The 2DGS blend is ratio * median_depth + (1 - ratio) * depth / alpha in the caller;
    train_ops.normal_consistency_loss(..., depth=median_depth, depth_alpha=(median_index >= 0).float()) takes the
    median depth's normals.  Whole single-GPU fp32 frames in the SH-precompute colour mode, Python orchestration,
    depth cut off: anything else raises RuntimeError (the trailing keyword arguments exist only to say so).
    antialiased, camera_model, filter3d: as rasterize()'s; median_depth stays the camera-frame z, not the distance along
    the ray."""
    fr, (uv, conic, opacity, rgb, z) = _begin_frame(
        gaussians, gaussians.sh, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
        background_rgb, "rasterize_median_depth", use_sh_precompute,
        (tile_rows is not None, return_aux, grad_sync, slab_sync, frame_hook), adam_plan=adam_plan,
        antialiased=antialiased, z_out=True, camera_model=camera_model, filter3d=filter3d)
    image, depth, alpha, median_depth, median_index = _Render.apply(uv, conic, opacity, rgb, z, fr, _MedianDepthMap)
    # visible -> dense numbering in one gather: -1 picks the sentinel behind the last visible row
    dense = torch.cat((fr.vis_idx, fr.vis_idx.new_full((1,), -1)))[median_index.long()]
    return image, depth, alpha, median_depth, dense, fr.culling_mask, uv


def rasterize_features(gaussians, features, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                       use_sh_precompute, background_rgb, tile_rows=None, return_aux=False, grad_sync=None,
                       slab_sync=None, frame_hook=None, adam_plan=None, antialiased=False,
                       camera_model="pinhole", filter3d=None):
    """rasterize() with a map of caller-supplied per-Gaussian feature vectors and the accumulated opacity:

        image, feature_map, alpha, culling_mask, uv = rasterize_features(gaussians, features, ...)

    features is [N, C] float32 on the Gaussians' device, 1 <= C <= 32, one row per Gaussian (dense: culled rows
    included; callers with more channels split them).  image, culling_mask and uv are those of rasterize() on the same
    inputs, bit for bit.  feature_map [H, W, C] = sum_k w_k features[k] with w_k = alpha_k T_k the compositing weights
    of the entries the colour forward walked; alpha [H, W] = sum_k w_k, bit-equal to rasterize_rgbd's.  No background
    term, no normalisation.  feature_map and alpha carry gradients to features (culled rows: exactly zero), to the
    Gaussians' parameters and, when it requires one, to camera_T_world (through the slab; features have no direct
    pose term); their backward is the true derivative (DESIGN.md "Feature maps").  Whole single-GPU fp32 frames in the
    SH-precompute colour mode, Python orchestration, depth cut off: anything else raises RuntimeError (the trailing
    keyword arguments exist only to say so).  antialiased, camera_model, filter3d: as rasterize()'s."""
    fr, (uv, conic, opacity, rgb) = _begin_frame(
        gaussians, gaussians.sh, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
        background_rgb, "rasterize_features", use_sh_precompute,
        (tile_rows is not None, return_aux, grad_sync, slab_sync, frame_hook), features, adam_plan,
        antialiased=antialiased, camera_model=camera_model, filter3d=filter3d)
    feat = _GatherRows.apply(features, fr.vis_idx.long()).contiguous()
    image, feature_map, alpha = _Render.apply(uv, conic, opacity, rgb, feat, fr, _FeatureMap)
    return image, feature_map, alpha, fr.culling_mask, uv


def rasterize_normals(gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                      use_sh_precompute, background_rgb, tile_rows=None, return_aux=False, grad_sync=None,
                      slab_sync=None, frame_hook=None, adam_plan=None, antialiased=False,
                      camera_model="pinhole", filter3d=None):
    """rasterize() with the two maps the normal-consistency regulariser of 2DGS reads, from one frame:

        image, depth, alpha, normal_map, culling_mask, uv = rasterize_normals(...)

    Each visible Gaussian's normal is the axis of its smallest log-scale (ties: the lowest index), rotated by its
    normalised quaternion and by the pose, and negated where it points away from the camera (n . xyz_cam > 0); the
    feature walk composites (n_x, n_y, n_z, z) with the frame's weights w_k = alpha_k T_k.  image, culling_mask and uv are
    those of rasterize(), depth [H, W] = sum w z and alpha [H, W] = sum w those of rasterize_rgbd() on the same inputs,
    bit for bit.  normal_map [H, W, 3] = sum w n is NOT normalised (2DGS's rend_normal); no background term.  All four
    maps carry gradients to the Gaussians' parameters -- z by rasterize_rgbd's route, the normals to the quaternion
    through gs_gaussian_normals_backward (the axis choice and the flip are constants: scale and xyz get nothing from
    them) -- and, when it requires one, to camera_T_world, the normals' rotation term included.
    depth_to_normal gives the other side of the loss, train_ops.normal_consistency_loss the loss itself.  Served like
    rasterize_features: whole single-GPU fp32 frames in the SH-precompute colour mode, Python orchestration, depth cut
    off; anything else raises RuntimeError before a kernel is enqueued (the trailing keyword arguments exist only to
    say so).  adam_plan is refused too: the fused optimizer step moves the quaternion inside the per-Gaussian backward,
    and the normals' quaternion gradient would arrive after it.  antialiased, camera_model, filter3d: as rasterize()'s
    (the normal itself does not depend on the projection model)."""
    _require(adam_plan is None, "rasterize_normals does not take the fused optimizer step (adam_plan): it steps the "
                                "quaternion inside the per-Gaussian backward, before the normals' gradient reaches it")
    g = gaussians
    fr, (uv, conic, opacity, rgb, z) = _begin_frame(
        g, g.sh, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
        background_rgb, "rasterize_normals", use_sh_precompute,
        (tile_rows is not None, return_aux, grad_sync, slab_sync, frame_hook), adam_plan=adam_plan,
        antialiased=antialiased, z_out=True, camera_model=camera_model, filter3d=filter3d)
    normals = _GaussianNormals.apply(g.quaternion.contiguous(), g.scale.contiguous(), camera_T_world.contiguous(), fr)
    feat = torch.cat((normals, z[:, None]), dim=1)
    image, feature_map, alpha = _Render.apply(uv, conic, opacity, rgb, feat, fr, _FeatureMap)
    return image, feature_map[..., 3], alpha, feature_map[..., :3], fr.culling_mask, uv


def depth_to_normal(depth, alpha, camera, camera_model="pinhole", min_alpha=0.0):
    """-> normal [H, W, 3] float32: the unit normal of the surface the depth map d = depth / alpha describes, from the
    central differences of the back-projected points, n = normalize((P(x, y+1) - P(x, y-1)) x (P(x+1, y) - P(x-1, y)))
    (2DGS's depth_to_normal orientation: towards the camera, like rasterize_normals' normals).  depth, alpha: float32
    [H, W] on the GPU, unnormalised as rasterize_rgbd / rasterize_normals / rasterize_distortion return them (a map that
    is a depth already, such as rasterize_median_depth's median_depth, goes in with alpha = its 0 / 1 validity,
    (median_index >= 0).float(): the quotient is the map itself); camera.K the
    frame's intrinsics; camera_model the frame's ("fisheye": P = d (tan(theta) / theta a, 1), a ray at or beyond 90
    degrees is invalid).  A pixel is valid when it is off the image's border, it and its four neighbours have
    alpha > min_alpha (>= 0) and a valid ray, and the cross product is not zero; invalid pixels are (0, 0, 0).
    Differentiable in depth and alpha with the validity held constant (gs_depth_normal / gs_depth_normal_backward;
    DESIGN.md 7l).  Anything else raises RuntimeError."""
    _require(camera_model in CAMERA_MODELS, f"camera_model must be one of {' / '.join(repr(m) for m in CAMERA_MODELS)}, "
                                            f"got {camera_model!r}")
    for name, t in (("depth", depth), ("alpha", alpha)):
        _require(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2,
                 f"depth_to_normal: {name} must be float32 [H, W] on the GPU (no fp64, no CPU path)")
    _require(alpha.shape == depth.shape and alpha.device == depth.device,
             f"depth_to_normal: alpha must match depth, got {list(alpha.shape)} and {list(depth.shape)}")
    K = camera.K
    _require(torch.is_tensor(K) and K.dtype == torch.float32 and K.device == depth.device and tuple(K.shape) == (3, 3),
             "depth_to_normal: camera.K must be float32 [3, 3] on the maps' device")
    min_alpha = float(min_alpha)
    _require(min_alpha >= 0.0, f"depth_to_normal: min_alpha must be a number >= 0, got {min_alpha}")
    mode = _hip.GS_RASTER_FISHEYE if camera_model == "fisheye" else _hip.GS_RASTER_CLASSIC
    return _DepthNormal.apply(depth.contiguous(), alpha.contiguous(), K.contiguous(), min_alpha, mode)


class ContributionStats:
    """How much each of the N Gaussians contributed to the frames swept into the record, from the blending weights
    w = alpha T of fused.rasterize_contributions:

        weight_sum  [N] float32   sum of w over the pixels and frames
        weight_max  [N] float32   largest w at any pixel of any frame
        pixel_count [N] int32     pixels the Gaussian contributed to, summed over the frames
        frames      int           frames accumulated

    `touched` is pixel_count > 0: the Gaussian reached at least one pixel (a frame's culling_mask is only the frustum
    test).  Passing the record back to rasterize_contributions adds the next view to it."""

    def __init__(self, weight_sum, weight_max, pixel_count, frames=0):
        self.weight_sum, self.weight_max, self.pixel_count, self.frames = weight_sum, weight_max, pixel_count, int(frames)

    @classmethod
    def zeros(cls, n, device):
        return cls(torch.zeros(n, dtype=torch.float32, device=device), torch.zeros(n, dtype=torch.float32, device=device),
                   torch.zeros(n, dtype=torch.int32, device=device), 0)

    @property
    def n(self):
        return int(self.weight_sum.shape[0])

    @property
    def touched(self):
        return self.pixel_count > 0

    def check(self, n, device=None):
        """raises unless the record is one of n Gaussians (on `device`) in the layout the kernel writes"""
        for name, t, dtype in (("weight_sum", self.weight_sum, torch.float32), ("weight_max", self.weight_max, torch.float32),
                               ("pixel_count", self.pixel_count, torch.int32)):
            _require(torch.is_tensor(t) and t.dim() == 1 and t.dtype == dtype and t.is_contiguous(),
                     f"ContributionStats.{name} must be a contiguous [N] {dtype} tensor")
            _require(t.shape[0] == n,
                     f"ContributionStats holds {t.shape[0]} Gaussians, the frame has {n}: statistics cannot be accumulated "
                     "across a change of N (start a new record after densification or pruning)")
            _require(device is None or t.device == device, f"ContributionStats.{name} is not on {device}")


def rasterize_contributions(gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                            use_sh_precompute, background_rgb, stats=None, antialiased=False, tile_rows=None,
                            return_aux=False, grad_sync=None, slab_sync=None, frame_hook=None, adam_plan=None,
                            camera_model="pinhole", filter3d=None):
    """rasterize() without gradients, with the per-Gaussian contribution statistics of the frame:

        image, stats, culling_mask = rasterize_contributions(gaussians, ...)                # a new record
        image, stats, culling_mask = rasterize_contributions(gaussians, ..., stats=stats)   # the next view, added to it

    image and culling_mask are those of rasterize() on the same inputs, bit for bit.  stats is a ContributionStats over
    all N Gaussians (culled rows: untouched): for every pixel and every entry the colour forward walked and found
    contributing, w = alpha T (the compositing weight, bit-equal to the one behind rasterize_rgbd's alpha) enters
    weight_sum, weight_max and pixel_count of its Gaussian.  One forward-only kernel on the frame's own lists
    (gs_render_contributions with row_index = the frame's visible indices): no [V] temporary, no scatter.  Runs under
    torch.no_grad(); nothing returned carries a gradient.  Whole single-GPU fp32 frames in the SH-precompute colour
    mode, Python orchestration, depth cut off: anything else raises RuntimeError before a kernel is enqueued (the
    trailing keyword arguments exist only to say so).  A stats of another N raises too.  antialiased, camera_model,
    filter3d: as rasterize()'s."""
    with torch.no_grad():
        n = int(gaussians.xyz.shape[0])
        if stats is not None:
            _require(isinstance(stats, ContributionStats), "rasterize_contributions: stats must be a ContributionStats")
            stats.check(n)
        fr, (_uv, _conic, _opacity, rgb) = _begin_frame(
            gaussians, gaussians.sh, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
            background_rgb, "rasterize_contributions", use_sh_precompute,
            (tile_rows is not None, return_aux, grad_sync, slab_sync, frame_hook), adam_plan=adam_plan,
            antialiased=antialiased, camera_model=camera_model, filter3d=filter3d)
        if stats is None:
            stats = ContributionStats.zeros(n, gaussians.xyz.device)
        else:
            stats.check(n, gaussians.xyz.device)
        image, nsp, _fw, _cost, _seg = fr.rendered if fr.rendered else render_forward(
            fr.packed, rgb, fr.ranges, fr.sorted_g, fr.keys, fr.background, fr.height, fr.width, None, fr.sort_prefix)
        if fr.vis_idx.shape[0] > 0:   # (nothing visible: nothing to add, and empty tensors have no address)
            contributions_forward(fr.packed, fr.ranges, fr.sorted_g, nsp, fr.height, fr.width, fr.vis_idx,
                                  stats.weight_sum, stats.weight_max, stats.pixel_count)
        stats.frames += 1
        return image.detach(), stats, fr.culling_mask


# ---------------------------------------------------------------------------------------------------
# 3D smoothing filter: the rate kernel, the filter from the rate, the baked export
# ---------------------------------------------------------------------------------------------------
def filter3d_rate(xyz, cameras_T_world, Ks, sizes, near_thresh=0.2, pad_fraction=0.15, camera_model="pinhole", out=None):
    """-> rate [N] float32: for every Gaussian the finest sampling rate, in pixels per world unit, of the cameras that see
    it (gs_filter3d_rate: one launch over all C cameras, xyz read once); 0 where no camera does.  cameras_T_world [C, 4, 4],
    Ks [C, 3, 3] float32 on xyz's device; sizes: (W, H) for all cameras, or an int tensor [C, 2].  A camera sees a
    Gaussian when z > near_thresh and uv lies inside the image padded by pad_fraction of its size on each side; its rate
    is max(fx, fy) / z, for camera_model="fisheye" max(fx, fy) / |xyz_cam| (the radial rate).  out: a rate to raise in
    place, so that calls over subsets of the cameras compose exactly.  The defaults are Mip-Splatting's."""
    _require(camera_model in CAMERA_MODELS, f"camera_model must be one of {' / '.join(repr(m) for m in CAMERA_MODELS)}, "
                                            f"got {camera_model!r}")
    _require(torch.is_tensor(xyz) and xyz.is_cuda and xyz.dtype == torch.float32 and xyz.dim() == 2 and xyz.shape[1] == 3,
             "filter3d_rate: xyz must be float32 [N, 3] on the GPU (no fp64, no CPU path)")
    dev, N = xyz.device, int(xyz.shape[0])
    _require(torch.is_tensor(cameras_T_world) and cameras_T_world.dim() == 3 and tuple(cameras_T_world.shape[1:]) == (4, 4),
             "filter3d_rate: cameras_T_world must be [C, 4, 4]")
    C = int(cameras_T_world.shape[0])
    _require(torch.is_tensor(Ks) and tuple(Ks.shape) == (C, 3, 3), f"filter3d_rate: Ks must be [{C}, 3, 3], one per camera")
    for name, t in (("cameras_T_world", cameras_T_world), ("Ks", Ks)):
        _require(t.dtype == torch.float32 and t.device == dev, f"filter3d_rate: {name} must be float32 on xyz's device")
    if torch.is_tensor(sizes):
        _require(tuple(sizes.shape) == (C, 2) and not sizes.is_floating_point(),
                 f"filter3d_rate: sizes must be (W, H) or an int tensor [{C}, 2]")
        sizes = sizes.to(device=dev, dtype=torch.int32).contiguous()
    else:
        W, H = (int(s) for s in sizes)
        sizes = torch.tensor([[W, H]], dtype=torch.int32, device=dev).repeat(C, 1)
    if out is None:
        out = torch.zeros(N, dtype=torch.float32, device=dev)
    else:
        _require(torch.is_tensor(out) and out.dtype == torch.float32 and out.device == dev and tuple(out.shape) == (N,)
                 and out.is_contiguous() and not out.requires_grad,
                 f"filter3d_rate: out must be a contiguous float32 [{N}] on xyz's device without a gradient")
    mode = _hip.GS_RASTER_FISHEYE if camera_model == "fisheye" else _hip.GS_RASTER_CLASSIC
    with torch.no_grad():
        _hip.call("gs_filter3d_rate", _p(xyz.contiguous()), _p(cameras_T_world.contiguous()), _p(Ks.contiguous()), _p(sizes),
                  C, N, near_thresh, pad_fraction, mode, _p(out), _stream())
    return out


def filter3d_from_rate(rate, variance=0.2):
    """-> phi [N] = variance / rate^2, the world-space variance of a `variance` px^2 low-pass at the Gaussian's finest
    sampling rate (Mip-Splatting: 0.2).  The rows no camera saw (rate == 0) take the largest phi of the rows that were
    seen; all zero when none was.  No host read."""
    seen = rate > 0
    lowest = torch.where(seen, rate, torch.full_like(rate, float("inf"))).amin() if rate.numel() else rate.new_zeros(())
    r = torch.where(seen, rate, lowest)          # (nothing seen: inf everywhere -> phi = 0)
    return variance / (r * r)


def bake_filter3d(gaussians, filter3d):
    """-> Gaussians with the filter folded into the parameters, for export to a renderer without one:
    scale' = 0.5 log(s^2 + phi), opacity' = logit(sigmoid(o) comp3) with comp3 = sqrt(prod_k s_k^2 / (s_k^2 + phi)); the
    other tensors are shared.  A classic frame of the result shows the filtered scene.  Plain torch on the tensors'
    device, differentiable; not for the training frame (rasterize(filter3d=) keeps the parameters unfiltered)."""
    from .splat_py.structs import Gaussians
    g = gaussians
    phi = filter3d.to(g.scale.dtype).reshape(-1, 1)
    s2 = torch.exp(g.scale) ** 2
    d = s2 + phi
    comp3 = torch.sqrt(torch.prod(s2 / d, dim=1, keepdim=True))
    opa3 = torch.sigmoid(g.opacity) * comp3
    return Gaussians(g.xyz, g.rgb, torch.log(opa3) - torch.log1p(-opa3), 0.5 * torch.log(d), g.quaternion, g.sh)
