"""Single-node multi-GPU rasterization: one frame sharded by tile rows (BASELINE.json north_star,
SURVEY.md 8(e)).  One process per GPU, torch.distributed over RCCL/xGMI (backend "nccl"); the same
code runs over gloo on CPU tensors for tests.

Per frame, on every rank (Gaussian parameters are replicated):
  forward   per-Gaussian stage for all N (cheap, replicated) -> binning, sort and render ONLY for the
            rank's band of tile rows -> all-gather of the band images (12 B/px of the own band
            out, ~13 MB in total at 1 MP).
  backward  every rank holds the same grad_image (the loss is evaluated on the gathered image on
            every rank); render backward over the rank's band gives PARTIAL per-Gaussian gradients
            (colour 3, opacity 1, uv 2, conic 3 floats: a Gaussian can straddle bands).  Then, by
            grad_mode:

  "replicated"  all-reduce(SUM) of that [V, 9] slab (36 B per visible Gaussian, ~100 MB at 2.86 M),
            per-Gaussian backward replicated -> identical dense parameter gradients on every rank.
            Same contract as the single-GPU function, but the all-reduce and the replicated
            backward bound the speed-up.
  "owner"   rank r owns the Gaussians of an index slice (owner_range) and produces the parameter
            gradients of that slice only, the way a sharded optimizer wants them.  The partial rows
            travel sparsely: every rank can tell from the replicated projection which bands a
            Gaussian reaches (HaloPlan), so ONE all_to_all moves a row only from a rank whose band
            the Gaussian reaches to the Gaussian's owner (~36 B x Gaussians-reaching-the-band per
            rank instead of 36 B x V), and the per-Gaussian backward runs on the owned slice.

Tile lists of a band equal the single-GPU lists restricted to the band (tested bit-exactly), so
the sharded image equals the single-GPU image bit for bit and gradients differ only by fp32
summation order.
"""
import ctypes

import torch
import torch.distributed as dist

from .splat_py.structs import Gaussians

DEFER_HOST_READ = True    # owner fused path: enqueue the render before waiting for the frame's counts
# owner mode, fused path, equal bands: the frame's orchestration in C++ (csrc/frame_hip.cpp: sharded_rasterize --
# the same two autograd nodes, the same C-ABI calls, the collectives through c10d); False keeps it in Python
NATIVE = True
# native path: evaluate the per-Gaussian stage in full only for the Gaussians that can reach the rank's band, into
# arrays compacted to those rows (csrc/preprocess.hip "band-compact"); False: every visible Gaussian, as on one GPU
BAND_COMPACT = True
OWNER_BLOCK = 256   # owner slices are whole blocks of the per-Gaussian kernels (csrc/halo.hip)
SLAB_WIDTH = 9      # rgb 3 | opacity 1 | uv 2 | conic 3


def band_rows_per_rank(n_tile_rows, world_size):
    return (n_tile_rows + world_size - 1) // world_size


def band_of(n_tile_rows, world_size, rank):
    """Contiguous split of the tile rows, [row0, row1) of `rank`: every band has
    ceil(rows / world_size) rows except the last ones, which take what is left (possibly nothing).
    Equal-sized bands let the image be all-gathered in place; the largest band -- which sets the
    frame time -- is as small as with any other contiguous split."""
    base = band_rows_per_rank(n_tile_rows, world_size)
    row0 = min(n_tile_rows, rank * base)
    return row0, min(n_tile_rows, row0 + base)


def balanced_bounds(row_cost, world_size):
    """Contiguous split of the tile rows into world_size bands that minimises the largest band cost
    ("cost-balanced by per-row splat counts"): binary search over the bound, greedy
    packing.  row_cost: one non-negative number per tile row.  -> world_size + 1 row boundaries
    (trailing bands may be empty).  Pure function of its arguments: every rank computes the same split
    from the same (all-gathered) costs."""
    cost = [max(0, int(c)) for c in row_cost]
    R = len(cost)

    def bands_needed(limit):
        n, acc = 1, 0
        for c in cost:
            if acc + c > limit and acc > 0:
                n, acc = n + 1, 0
            acc += c
        return n

    lo, hi = max(cost + [0]), sum(cost)
    while lo < hi:
        mid = (lo + hi) // 2
        if bands_needed(mid) <= world_size:
            hi = mid
        else:
            lo = mid + 1
    bounds, acc = [0], 0
    for r, c in enumerate(cost):
        if acc + c > lo and acc > 0 and len(bounds) < world_size:
            bounds.append(r)
            acc = 0
        acc += c
    bounds += [R] * (world_size + 1 - len(bounds))
    return bounds


def owner_blocks(N, world_size):
    """Boundaries, in blocks of OWNER_BLOCK Gaussians, of the index slices the ranks own."""
    nb = (max(N, 1) + OWNER_BLOCK - 1) // OWNER_BLOCK
    return [(nb * r) // world_size for r in range(world_size + 1)]


def owner_range(N, world_size, rank):
    """[i0, i1): the Gaussians whose parameter gradients `rank` produces in grad_mode "owner"."""
    b = owner_blocks(N, world_size)
    return min(N, OWNER_BLOCK * b[rank]), min(N, OWNER_BLOCK * b[rank + 1])


def owned_slice(gaussians, world_size, rank, requires_grad=True):
    """Leaf copies of the slice of every parameter that `rank` owns (what a sharded optimizer holds)."""
    i0, i1 = owner_range(gaussians.xyz.shape[0], world_size, rank)

    def cut(t):
        return None if t is None else t.detach()[i0:i1].clone().requires_grad_(requires_grad)

    g = gaussians
    return Gaussians(cut(g.xyz), cut(g.rgb), cut(g.opacity), cut(g.scale), cut(g.quaternion), cut(g.sh))


# ---------------------------------------------------------------------------------------------------
# sparse exchange of the partial render gradients
# ---------------------------------------------------------------------------------------------------
class HaloPlan:
    """Who sends which rows of the [V, 9] slab to whom, for one frame and one rank (csrc/halo.hip).

    mask[v] bit s: visible Gaussian v reaches the band of rank s.  The send buffer of this rank is
    slab[send_index] (visible indices with this rank's bit, ascending == grouped by owner),
    send_splits[r] rows for owner r; from sender s this rank receives recv_splits[s] rows: its own
    visible range [v_lo, v_hi) restricted to bit s, ascending."""

    def __init__(self, world_size, rank, mask, send_index, send_splits, recv_splits, v_lo, v_hi, hip=None):
        self.world_size, self.rank = world_size, rank
        self.mask, self.send_index = mask, send_index
        self.send_splits, self.recv_splits = list(send_splits), list(recv_splits)
        self.v_lo, self.v_hi = v_lo, v_hi
        self.hip = hip   # (N, workspace) when built by gs_halo_plan

    @staticmethod
    def reference(mask, v_bounds, world_size, rank):
        """Plain-PyTorch construction from the masks of the visible Gaussians and the visible-index
        bounds of the owner slices (any device; the checker of the HIP construction and the plan of
        the reference-shaped path)."""
        bit = (mask >> rank) & 1
        send_index = torch.nonzero(bit, as_tuple=False).flatten()
        bounds = torch.as_tensor(v_bounds, device=send_index.device)
        cuts = torch.searchsorted(send_index, bounds).tolist()
        send_splits = [cuts[r + 1] - cuts[r] for r in range(world_size)]
        v_lo, v_hi = int(v_bounds[rank]), int(v_bounds[rank + 1])
        mine = mask[v_lo:v_hi]
        recv_splits = [int(((mine >> s) & 1).sum()) for s in range(world_size)]
        return HaloPlan(world_size, rank, mask, send_index, send_splits, recv_splits, v_lo, v_hi)

    def pack(self, slab):
        return slab.index_select(0, self.send_index)

    def unpack(self, recv):
        """[sum(recv_splits), 9] -> the summed rows of the owned visible range [v_hi - v_lo, 9]"""
        n = self.v_hi - self.v_lo
        # the HIP kernel writes every row of the range; the index_add form accumulates onto zeros
        alloc = torch.empty if self.hip is not None else torch.zeros
        out = alloc(max(n, 1), SLAB_WIDTH, dtype=recv.dtype, device=recv.device)[:n]
        if n == 0:
            return out
        if self.hip is not None:
            from . import _hip
            N, workspace = self.hip
            off, offsets = 0, []
            for c in self.recv_splits:
                offsets.append(off)
                off += c
            offs = (ctypes.c_int32 * len(offsets))(*offsets)
            p = _hip.ptr
            _hip.call("gs_halo_gather_sum", p(self.mask), p(workspace), N, self.world_size, self.rank, self.v_lo,
                      self.v_hi, p(recv), offs, p(out), _hip.current_stream())
            return out
        mine = self.mask[self.v_lo:self.v_hi]
        off = 0
        for s, c in enumerate(self.recv_splits):
            idx = torch.nonzero((mine >> s) & 1, as_tuple=False).flatten()
            out.index_add_(0, idx, recv[off:off + c])
            off += c
        return out

    def exchange(self, slab, group=None, all_to_all=None):
        """partial slab [V, 9] of this rank's band -> summed rows of the owned visible range"""
        send = self.pack(slab).contiguous()
        recv = torch.empty(sum(self.recv_splits), SLAB_WIDTH, dtype=slab.dtype, device=slab.device)
        if all_to_all is not None:
            all_to_all(recv, send, self.recv_splits, self.send_splits)
        elif slab.is_cuda:
            from . import _hip
            _hip.timed_region("rccl_all_to_all_grad_rows", lambda: dist.all_to_all_single(
                recv, send, self.recv_splits, self.send_splits, group=group))
        else:
            dist.all_to_all_single(recv, send, self.recv_splits, self.send_splits, group=group)
        return self.unpack(recv)


def _band_rows(n_tile_rows, world_size):
    return [band_of(n_tile_rows, world_size, r)[0] for r in range(world_size)] + [n_tile_rows]


def plan_record_ints(world_size):
    return 4 + 2 * world_size


def enqueue_hip_plan(f, world_size, rank, bounds=None):
    """preprocess_forward's `plan` hook: enqueues gs_halo_plan; the device record f.record
    (rows to send, V, v_lo, v_hi, send[G], recv[G]) rides on the frame's one host read, and the
    send list -- the visible Gaussians whose window reaches this rank's band -- doubles as the
    subset the binning walks."""
    from . import _hip
    G = world_size
    n_ws = _hip.lib().gs_halo_workspace_ints(f.N, G)
    buf = torch.empty(2 * f.N + n_ws, dtype=torch.int32, device=f.uv.device)
    f.halo_mask, f.halo_send_index, f.halo_ws = buf[:f.N], buf[f.N:2 * f.N], buf[2 * f.N:]
    rows = (ctypes.c_int32 * (G + 1))(*(bounds if bounds is not None else _band_rows(f.nty, G)))
    blks = (ctypes.c_int32 * (G + 1))(*owner_blocks(f.N, G))
    p = _hip.ptr
    _hip.call("gs_halo_plan", p(f.uv), p(f.conic), f.N, p(f.count), p(f.ws), f.ntx, f.nty, f.mh_dist, rows, blks, G, rank,
              p(f.halo_mask), p(f.halo_ws), p(f.halo_send_index), p(f.record), f.stream)
    if G > 1:
        f.subset = (f.halo_send_index, f.record)   # record[0] = length of the list


def finish_hip_plan(f, world_size, rank):
    G = world_size
    h = f.host
    send_splits, recv_splits = h[4:4 + G], h[4 + G:4 + 2 * G]
    return HaloPlan(G, rank, f.halo_mask, f.halo_send_index[:sum(send_splits)], send_splits, recv_splits,
                    h[2], h[3], hip=(f.N, f.halo_ws))


# ---------------------------------------------------------------------------------------------------
# autograd pieces
# ---------------------------------------------------------------------------------------------------
def gather_bands(image, band_pixels, world_size, rank, group=None):
    """image [>= world_size * band_pixels / W rows, W, 3] holding this rank's band at rows
    [rank * band, (rank + 1) * band): all-gather so that every rank holds every band (12 B/px of
    the own band out, the rest in -- 1/8 of an all-reduce's traffic at 8 ranks)."""
    flat = image.view(-1)[:world_size * band_pixels]
    mine = flat[rank * band_pixels:(rank + 1) * band_pixels].clone()
    if image.is_cuda:
        from . import _hip
        _hip.timed_region("rccl_all_gather_image", lambda: dist.all_gather_into_tensor(flat, mine, group=group))
    else:
        dist.all_gather_into_tensor(flat, mine, group=group)
    return image


class _GatherImage(torch.autograd.Function):
    """forward: all-gather of the band images; backward: identity, because every rank evaluates
    the same loss on the same gathered image (see ShardedRasterizer: the loss contract)."""

    @staticmethod
    def forward(ctx, image, rast):
        H, W = image.shape[0], image.shape[1]
        rows = rast.buffer_rows()
        out = torch.zeros(rows, W, 3, dtype=image.dtype, device=image.device)
        out[:H] = image
        return rast.gather(out, H)

    @staticmethod
    def backward(ctx, grad):
        return grad, None


class _SumGradsAcrossRanks(torch.autograd.Function):
    """identity in forward; in backward the partial per-Gaussian render gradients of all bands are
    summed with ONE all-reduce over a flat slab."""

    @staticmethod
    def forward(ctx, group, *tensors):
        ctx.group = group
        return tuple(t.view_as(t) for t in tensors)

    @staticmethod
    def backward(ctx, *grads):
        shapes = [g.shape for g in grads]
        flat = torch.cat([g.reshape(-1) for g in grads])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=ctx.group)
        out, off = [], 0
        for s in shapes:
            n = s.numel()
            out.append(flat[off:off + n].view(s))
            off += n
        return (None,) + tuple(out)


class _OwnerExchange(torch.autograd.Function):
    """Reference-shaped path, grad_mode "owner": identity in forward; in backward the partial
    gradients (rgb [V,3], opacity [V,1], uv [V,2], conic [V,3]) become complete for the visible
    Gaussians this rank owns (sparse all_to_all) and zero elsewhere, so the dense per-Gaussian
    backward that follows is exact on the owned slice."""

    @staticmethod
    def forward(ctx, rast, plan_of, rgb, opacity, uv, conic):
        ctx.rast, ctx.plan_of = rast, plan_of
        return rgb.view_as(rgb), opacity.view_as(opacity), uv.view_as(uv), conic.view_as(conic)

    @staticmethod
    def backward(ctx, g_rgb, g_opacity, g_uv, g_conic):
        plan = ctx.plan_of()
        slab = torch.cat([g_rgb, g_opacity, g_uv, g_conic], dim=1).contiguous()
        owned = plan.exchange(slab, group=ctx.rast.group)
        full = torch.zeros_like(slab)
        full[plan.v_lo:plan.v_hi] = owned
        return None, None, full[:, 0:3], full[:, 3:4], full[:, 4:6], full[:, 6:9]


class _OwnerPreprocess(torch.autograd.Function):
    """First node of the owner-mode frame on the fused HIP path: per-Gaussian stage for all N, halo plan,
    binning and sort of the rank's band.  The owned parameter slices are the differentiable inputs (they
    receive the gradients), the replicated full tensors provide the values.  Output: uv (so that
    uv.retain_grad() / uv.grad work as in the single-GPU function, trainer.py:360,379) and the culling
    mask; everything else travels to the render node in the frame record `fr`."""

    @staticmethod
    def forward(ctx, o_xyz, o_quaternion, o_scale, o_opacity, o_rgb, o_sh, rast, fr, g, camera_T_world, K, width,
                height, near_thresh, far_thresh, cull_mask_padding, mh_dist, background_rgb):
        from . import _hip, fused
        G, me = rast.world_size, rast.rank
        sort_prefix = _hip.GS_SORT_PREFIX if fused.SORT_PREFIX else 0
        full = tuple(None if t is None else (t if t.is_contiguous() else t.contiguous())
                     for t in (g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh))   # values only (no_grad here)
        bounds = list(rast.bounds)
        tile_rows = fr.tile_rows = rast.tile_rows   # this frame's band, whatever a later rasterize() makes of rast.bounds
        f = fused.preprocess_forward(*full, camera_T_world, K, width, height, near_thresh, far_thresh,
                                     cull_mask_padding, mh_dist, tile_rows, sort_prefix,
                                     plan=lambda frm: enqueue_hip_plan(frm, G, me, bounds),
                                     plan_ints=plan_record_ints(G), defer=True)
        if not DEFER_HOST_READ:
            fused.preprocess_finish(f)

        def render(exact_count):
            seg = fused.segments_for(f.hint_key, f.S if exact_count else f.sorted_buf.shape[0], exact_count,
                                     (f.row1 - f.row0) * f.ntx)
            return fused.render_forward(f.packed, f.rgb_render, f.ranges, f.sorted_buf, f.keys_buf, background_rgb,
                                        height, width, tile_rows, sort_prefix, image_rows=rast.buffer_rows(),
                                        segments=seg)

        # the render is enqueued on the speculative tile lists before the host looks at the frame's
        # counts, so the GPU does not wait for the host; a too small capacity repeats it (rare)
        out = render(False) if (f.speculative and DEFER_HOST_READ and sort_prefix and f.capacity > sort_prefix) else None
        if (DEFER_HOST_READ and fused.preprocess_finish(f)) or out is None:
            out = render(True)
        fr.f, fr.rendered, fr.plan = f, out, finish_hip_plan(f, G, me)
        fr.full, fr.cam, fr.background = full, (camera_T_world, K), background_rgb
        rast.last_plan = fr.plan
        ctx.fr, ctx.rast = fr, rast
        ctx.set_materialize_grads(False)
        uv = f.uv[:f.V]
        ctx.mark_non_differentiable(f.culling_mask)
        return uv, f.culling_mask

    @staticmethod
    def backward(ctx, g_uv, *unused):
        # g_uv is what _OwnerRender.backward handed to uv (it fills uv.grad); the rows the per-Gaussian
        # backward needs are the exchanged ones it left in the frame record
        from . import fused
        fr, rast = ctx.fr, ctx.rast
        if fr.owned_rows is None:
            return (None,) * 18
        f, plan = fr.f, fr.plan
        camera_T_world, K = fr.cam
        i0, i1 = owner_range(f.N, rast.world_size, rast.rank)
        # a loss term applied directly to the returned uv arrives here on top of what _OwnerRender.backward
        # handed over: g_uv = (render rows of the owned Gaussians | the stride-0 zero placeholder) + that
        # term; the render part is already in owned_rows, the rest is added for the owned rows (every rank
        # evaluates the same loss, so each owner takes its own slice -- as in the replicated mode)
        rendered = fr.rendered_uv_grad
        fr.rendered_uv_grad = None
        if g_uv is not None and g_uv is not rendered and g_uv.stride() != (0, 0) and plan.v_hi > plan.v_lo:
            extra = g_uv[plan.v_lo:plan.v_hi]
            if rendered is not None and rendered.stride() != (0, 0):
                extra = extra - rendered[plan.v_lo:plan.v_hi]
            fr.owned_rows = fr.owned_rows.clone()
            fr.owned_rows[:, 4:6] += extra
        grads = fused.preprocess_backward(fr.full[0], fr.full[1], fr.full[2], camera_T_world, K, f, fr.owned_rows,
                                          v_base=plan.v_lo, i0=i0, i1=i1)
        fr.owned_rows = None
        return grads + (None,) * 12


class _OwnerRender(torch.autograd.Function):
    """Second node: the band's image (already enqueued by _OwnerPreprocess.forward) -> all-gather.
    Backward: render backward over the band, sparse exchange of the partial rows to their owners; the
    gradient returned for uv holds the complete render-backward grad_uv of the Gaussians this rank owns
    (rows [v_lo, v_hi)) and zeros elsewhere -- materialised only when somebody asked for uv.grad."""

    @staticmethod
    def forward(ctx, uv, rast, fr, height, width):
        image, nsp, fw, cost, seg = fr.rendered
        fr.rendered = None
        f = fr.f
        V = f.V
        ctx.save_for_backward(f.packed, f.rgb_render[:V], f.ranges, f.sorted_g, fr.background, nsp, fw, cost, seg)
        ctx.fr, ctx.rast, ctx.dims = fr, rast, (height, width)
        # the band and the gradient mode of THIS frame: under band_policy="cost" rast.tile_rows moves with every
        # rasterize() call, and a second forward before this frame's backward (an eval render, gradient
        # accumulation over views) must not change the rows the backward covers
        from . import _hip
        ctx.tile_rows = fr.tile_rows
        ctx.backward_mode = _hip.get_backward_mode()
        ctx.set_materialize_grads(False)
        return rast.gather(image, height, ranges=f.ranges, ntx=f.ntx)

    @staticmethod
    def backward(ctx, grad_image):
        from . import fused
        if grad_image is None:
            return (None,) * 5
        packed, rgb_v, ranges, sorted_g, background_rgb, nsp, fw, cost, seg = ctx.saved_tensors
        fr, rast = ctx.fr, ctx.rast
        f, plan = fr.f, fr.plan
        height, width = ctx.dims
        slab = fused.render_backward(packed, rgb_v, ranges, sorted_g, background_rgb, nsp, fw,
                                     grad_image.contiguous(), height, width, ctx.tile_rows, f.V, cost,
                                     ctx.backward_mode, seg)
        owned = plan.exchange(slab, group=rast.group, all_to_all=rast.all_to_all)
        rast.last_owned_render_grads = fr.owned_rows = owned
        uv_out = fr.uv_ref() if fr.uv_ref is not None else None
        if uv_out is not None and uv_out.retains_grad:
            g_uv = torch.zeros(f.V, 2, dtype=owned.dtype, device=owned.device)
            g_uv[plan.v_lo:plan.v_hi] = owned[:, 4:6]
        else:   # nobody reads uv.grad: a stride-0 zero costs nothing and still routes the backward
            g_uv = torch.zeros(1, dtype=owned.dtype, device=owned.device).expand(f.V, 2)
        fr.rendered_uv_grad = g_uv   # _OwnerPreprocess.backward tells it from a gradient a loss put on uv
        return g_uv, None, None, None, None


class _OwnerFrameGeneric(torch.autograd.Function):
    """grad_mode "owner" over the reference-shaped path (any dtype / colour mode, CPU tensors in the
    tests): the frame's graph is built on replicated leaf copies, the sparse exchange completes the
    render gradients of the owned Gaussians, and the owned rows of the dense gradients are handed to
    the owned parameter slices."""

    @staticmethod
    def forward(ctx, o_xyz, o_quaternion, o_scale, o_opacity, o_rgb, o_sh, rast, g, camera_T_world, camera, args,
                background_rgb):
        from . import backend
        from .splat_py.rasterize import rasterize as impl
        near_thresh, far_thresh, cull_mask_padding, mh_dist, use_sh_precompute = args
        G, me = rast.world_size, rast.rank
        names = ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")
        state = {}

        def plan_of():
            return state["plan"]

        def sync(rgb, opacity, uv, conic):
            if rgb.dim() != 2:   # per-pixel SH colour: [V, 3, n_sh] rows do not fit the 9-wide slab
                return _SumGradsAcrossRanks.apply(rast.group, rgb, opacity, uv, conic)
            ntx, nty = (camera.width + 15) // 16, (camera.height + 15) // 16
            mask = backend.get().band_mask(uv.detach().contiguous(), conic.detach().contiguous(), ntx, nty,
                                           mh_dist, list(rast.bounds))
            state["mask"] = mask
            return _OwnerExchange.apply(rast, plan_of, rgb, opacity, uv, conic)

        with torch.enable_grad():
            rep = Gaussians(*[None if getattr(g, k) is None else getattr(g, k).detach().clone().requires_grad_(True)
                              for k in ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")])
            image, culling_mask, uv = impl(rep, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding,
                                           mh_dist, use_sh_precompute, background_rgb, tile_rows=rast.tile_rows,
                                           grad_sync=sync)
        N = g.xyz.shape[0]
        if "mask" in state:
            keep = ~culling_mask
            prefix = torch.cumsum(keep.to(torch.int64), 0)
            v_bounds = [0 if i == 0 else int(prefix[i - 1])
                        for i in (min(N, OWNER_BLOCK * b) for b in owner_blocks(N, G))]
            state["plan"] = HaloPlan.reference(state["mask"], v_bounds, G, me)
            rast.last_plan = state["plan"]
        ctx.rep, ctx.local_image, ctx.names = rep, image, names
        ctx.range = owner_range(N, G, me)
        out = _GatherImage.forward(None, image.detach(), rast)
        uv_out = uv.detach()
        ctx.mark_non_differentiable(culling_mask, uv_out)
        return out, culling_mask, uv_out

    @staticmethod
    def backward(ctx, grad_image, *unused):
        torch.autograd.backward(ctx.local_image, grad_image)
        i0, i1 = ctx.range
        rep = ctx.rep
        order = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
        grads = tuple(None if getattr(rep, k) is None else getattr(rep, k).grad[i0:i1] for k in order)
        return grads + (None,) * 6


class ShardedRasterizer:
    """One rank of the tile-row sharded frame.

    Loss contract: the returned image is the full frame on every rank and its backward is the identity
    (no collective): every rank must evaluate the SAME, un-averaged loss on it, so that every rank feeds
    the same grad_image into its band's render backward.  A per-rank loss (DDP-style: a different target
    or a 1/world_size factor per rank) gives gradients that are silently wrong; `check_grad_image=True`
    verifies the contract with one extra all-reduce per backward (debugging aid).

    band_policy "equal": ceil(rows / world_size) tile rows per rank (in-place all-gather).
    band_policy "cost": contiguous bands balanced by per-row cost (balanced_bounds) -- the previous
    frame's per-row instance counts, which ride on the image all-gather (fused path), or costs given
    with set_row_costs(); applies from the next frame on, identically on every rank."""

    TILE_COST = 64   # per-tile constant of the row cost (a tile with an empty list still costs a workgroup)

    def __init__(self, image_height, world_size=None, rank=None, group=None, fused=True, grad_mode="replicated",
                 all_to_all=None, band_policy="equal", check_grad_image=False, native=None):
        if grad_mode not in ("replicated", "owner"):
            raise ValueError("grad_mode must be 'replicated' or 'owner'")
        if band_policy not in ("equal", "cost"):
            raise ValueError("band_policy must be 'equal' or 'cost'")
        self.group = group
        self.world_size = world_size if world_size is not None else dist.get_world_size(group)
        self.rank = rank if rank is not None else dist.get_rank(group)
        self.fused = fused
        self.grad_mode = grad_mode
        self.band_policy = band_policy
        self.check_grad_image = check_grad_image
        self.native = native   # None: the module default NATIVE; False: this rasterizer keeps the Python orchestration
        self.all_to_all = all_to_all   # test hook: stands in for dist.all_to_all_single (and skips the image gather)
        self.n_tile_rows = (image_height + 15) // 16
        self.bounds = _band_rows(self.n_tile_rows, self.world_size)
        # pixel rows of a (full) equal band, and of an image buffer that holds world_size of them
        self.band_pixel_rows = 16 * band_rows_per_rank(self.n_tile_rows, self.world_size)
        self.padded_height = self.band_pixel_rows * self.world_size
        self.last_plan = None
        self.last_owned_render_grads = None
        self._pending_costs = None   # (pinned host tensor, event) of the latest gathered row costs
        self._row_map = {}

    # ---- bands -----------------------------------------------------------------------------------------
    @property
    def tile_rows(self):
        return self.bounds[self.rank], self.bounds[self.rank + 1]

    def set_row_costs(self, row_cost):
        """cost policy: new band boundaries from per-tile-row costs (the same numbers on every rank)"""
        if self.band_policy == "cost":
            self.bounds = balanced_bounds(row_cost, self.world_size)

    def _update_bounds(self):
        """cost policy: consume the row costs the previous frame's gather left behind (the copy to the
        host was enqueued then; the event has long passed by now, so this does not stall)"""
        if self.band_policy != "cost" or self._pending_costs is None:
            return
        host, event = self._pending_costs
        self._pending_costs = None
        if event is not None:
            event.synchronize()
        self.set_row_costs(host.tolist())

    def chunk_rows(self):
        """pixel rows of one rank's part of the image all-gather"""
        if self.band_policy == "equal":
            return self.band_pixel_rows
        return 16 * max(self.bounds[r + 1] - self.bounds[r] for r in range(self.world_size)) + 1   # + 1: the cost row

    def buffer_rows(self):
        """pixel rows of the buffer a band is rendered into (the band sits at its own rows)"""
        if self.band_policy == "equal":
            return self.padded_height
        return 16 * self.n_tile_rows + self.chunk_rows()

    def owned_range(self, N):
        return owner_range(N, self.world_size, self.rank)

    # ---- image gather -----------------------------------------------------------------------------------
    def gather(self, image, height, ranges=None, ntx=None):
        """image: [buffer_rows(), W, 3] holding this rank's band at its own pixel rows -> the full frame
        [height, W, 3] on every rank.  ranges/ntx (fused path, cost policy): the band's tile ranges, from
        which the per-row costs for the next frame's bands are formed and sent along."""
        if self.all_to_all is not None:   # simulated ranks (tests): the caller sums the band images
            return image[:height]
        W = image.shape[1]
        if self.band_policy == "equal":
            gather_bands(image, self.band_pixel_rows * W * 3, self.world_size, self.rank, self.group)
            return image[:height]
        G, R = self.world_size, self.n_tile_rows
        row0, row1 = self.tile_rows
        crows = self.chunk_rows()
        if R > W * 3:
            raise ValueError("image too narrow for the cost row")
        tail = image[16 * row0 + crows - 1].view(-1)   # the chunk's last pixel row carries the row costs
        tail[:R] = 0
        if ranges is not None and row1 > row0:
            counts = (ranges[row0 * ntx + 1:row1 * ntx + 1] - ranges[row0 * ntx:row1 * ntx]).clamp(max=1024)
            tail[row0:row1] = (counts.view(row1 - row0, ntx).sum(1) + self.TILE_COST * ntx).to(image.dtype)
        mine = image[16 * row0:16 * row0 + crows].reshape(-1)
        out = torch.empty(G * mine.numel(), dtype=image.dtype, device=image.device)
        if image.is_cuda:
            from . import _hip
            _hip.timed_region("rccl_all_gather_image", lambda: dist.all_gather_into_tensor(out, mine, group=self.group))
        else:
            dist.all_gather_into_tensor(out, mine, group=self.group)
        out = out.view(G * crows, W, 3)
        key = tuple(self.bounds)
        row_map = self._row_map.get(key)
        if row_map is None:
            idx = []
            for r in range(G):
                idx += [r * crows + y for y in range(min(height, 16 * self.bounds[r + 1]) - 16 * self.bounds[r])]
            row_map = torch.tensor(idx, dtype=torch.int64, device=image.device)
            self._row_map = {key: row_map}
        full = out.index_select(0, row_map)
        if ranges is not None:
            costs = out.view(G, crows, W * 3)[:, crows - 1, :R].sum(0)
            host = torch.empty(R, dtype=costs.dtype, pin_memory=image.is_cuda)
            host.copy_(costs, non_blocking=True)
            event = None
            if image.is_cuda:
                event = torch.cuda.Event()
                event.record()
            self._pending_costs = (host, event)
        return full

    def gather_image_(self, image):
        """(kept for callers of the first version) equal bands, in place"""
        return self.gather(image, image.shape[0])

    # ---- gradient synchronisation -------------------------------------------------------------------------
    def _grad_sync(self, *tensors):
        return _SumGradsAcrossRanks.apply(self.group, *tensors)

    def _slab_sync(self, flat):
        if flat.is_cuda:
            from . import _hip
            _hip.timed_region("rccl_all_reduce_grad_slab",
                              lambda: dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group))
        else:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)

    def _checked(self, image):
        return _CheckGradImage.apply(image, self) if self.check_grad_image and self.all_to_all is None else image

    def rasterize(self, gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                  use_sh_precompute, background_rgb, owned=None):
        """Same contract as splat_py.rasterize.rasterize; the returned image is the full frame on
        every rank.  grad_mode "owner": `gaussians` holds the replicated values, `owned` (see
        owned_slice) the leaf tensors of this rank's slice, which receive the gradients; uv.grad (after
        uv.retain_grad()) then holds the complete rows of the owned Gaussians and zeros elsewhere."""
        import weakref
        from types import SimpleNamespace

        from . import fused
        self._update_bounds()
        use_fused = self.fused and fused.supported(gaussians, camera_T_world, camera, use_sh_precompute)
        if use_fused:
            fused.validate(gaussians, camera_T_world, camera, background_rgb)
        if self.grad_mode == "owner":
            if owned is None:
                raise ValueError("grad_mode 'owner' needs owned= (the parameter slices of this rank)")
            o = (owned.xyz, owned.quaternion, owned.scale, owned.opacity, owned.rgb, owned.sh)
            use_native = NATIVE if self.native is None else self.native
            nat = fused.native() if (use_fused and use_native) else None
            if nat is not None and self.band_policy == "cost":
                # the costs the previous frame's image gather left in pinned memory (csrc/frame_hip.cpp) -> this frame's bands
                costs = nat.take_row_costs()
                if costs is not None:
                    self.set_row_costs(costs)
            if nat is not None:
                g = gaussians
                nat.set_modes(bool(fused.SORT_PREFIX), bool(fused.EARLY_RENDER))
                nat.set_segments(0 if fused.SEGMENTS == "auto" else (1 if fused.SEGMENTS else -1))
                nat.set_band_compact(bool(BAND_COMPACT))
                group = None
                if self.all_to_all is None:
                    group = self.group if self.group is not None else dist.group.WORLD
                image, culling_mask, uv = nat.sharded_rasterize(
                    *o, g.xyz, g.quaternion, g.scale, g.opacity, g.rgb, g.sh, camera_T_world, camera.K, int(camera.width),
                    int(camera.height), near_thresh, far_thresh, cull_mask_padding, mh_dist, background_rgb,
                    self.world_size, self.rank, list(self.bounds), owner_blocks(g.xyz.shape[0], self.world_size), group,
                    self.all_to_all, self.band_policy == "cost")
                p = nat.last_plan()
                self.last_plan = SimpleNamespace(send_splits=p["send_splits"], recv_splits=p["recv_splits"],
                                                 v_lo=p["v_lo"], v_hi=p["v_hi"])
                return self._checked(image), culling_mask, uv
            if use_fused:
                fr = SimpleNamespace(owned_rows=None, uv_ref=None, rendered_uv_grad=None, tile_rows=None)
                uv, culling_mask = _OwnerPreprocess.apply(
                    *o, self, fr, gaussians, camera_T_world.contiguous(), camera.K.contiguous(), int(camera.width),
                    int(camera.height), near_thresh, far_thresh, cull_mask_padding, mh_dist,
                    background_rgb.contiguous())
                fr.uv_ref = weakref.ref(uv)
                image = _OwnerRender.apply(uv, self, fr, int(camera.height), int(camera.width))
                return self._checked(image), culling_mask, uv
            image, culling_mask, uv = _OwnerFrameGeneric.apply(
                *o, self, gaussians, camera_T_world, camera,
                (near_thresh, far_thresh, cull_mask_padding, mh_dist, use_sh_precompute), background_rgb)
            return self._checked(image), culling_mask, uv
        if use_fused:
            impl = fused.rasterize
        else:
            from .splat_py.rasterize import rasterize as impl
        hook = {}
        image, culling_mask, uv = impl(
            gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
            use_sh_precompute, background_rgb, tile_rows=self.tile_rows, grad_sync=self._grad_sync,
            **({"slab_sync": self._slab_sync, "frame_hook": hook.update} if use_fused else {}))
        image = _GatherImage.apply(image, self) if "ranges" not in hook else _GatherImageCost.apply(image, self, hook)
        return self._checked(image), culling_mask, uv


class _GatherImageCost(torch.autograd.Function):
    """_GatherImage that also sends the band's per-row costs along (fused path, replicated gradients)"""

    @staticmethod
    def forward(ctx, image, rast, hook):
        H, W = image.shape[0], image.shape[1]
        out = torch.zeros(rast.buffer_rows(), W, 3, dtype=image.dtype, device=image.device)
        out[:H] = image
        return rast.gather(out, H, ranges=hook["ranges"], ntx=hook["ntx"])

    @staticmethod
    def backward(ctx, grad):
        return grad, None, None


class _CheckGradImage(torch.autograd.Function):
    """identity; in backward asserts that every rank received the same grad_image (the loss contract of
    ShardedRasterizer) -- one all-reduce of a checksum, debugging aid"""

    @staticmethod
    def forward(ctx, image, rast):
        ctx.rast = rast
        return image.view_as(image)

    @staticmethod
    def backward(ctx, grad):
        rast = ctx.rast
        s = torch.stack([grad.double().sum(), grad.double().abs().sum()])
        lo, hi = s.clone(), s.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=rast.group)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=rast.group)
        if not torch.equal(lo, hi):
            raise RuntimeError("ShardedRasterizer: grad_image differs between ranks -- every rank must evaluate "
                               "the same un-averaged loss on the gathered image")
        return grad, None
