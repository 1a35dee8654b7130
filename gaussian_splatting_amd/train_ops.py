"""Training-loop operations right behind the rasterizer, over the C ABI.

    Adam                      drop-in for the torch.optim.Adam the reference builds in
                              splat_py/optimizer_manager.py:15-42 and steps in trainer.py:376: same
                              constructor, param_groups and state layout ("step", "exp_avg",
                              "exp_avg_sq"), so OptimizerManager's parameter surgery works on it
                              unchanged; step() is ONE HIP launch over all parameter tensors
    FusedRasterAdam           Adam whose rasterize() returns a frame that steps quaternion, scale, opacity,
                              rgb and sh INSIDE its backward (the per-Gaussian backward kernel applies the
                              update where the gradients are in registers: they are never written out and
                              read back); step() then steps xyz.  Opt-in; falls back to fused.rasterize +
                              Adam.step whenever a condition of the fused step does not hold
    SelectiveAdam             Adam whose step(culling_mask=...) steps only the Gaussians the frame saw (the
                              `sparse_adam` / SelectiveAdam of other trainers): a culled row's parameters and
                              moments are neither read nor written; one HIP launch (gs_adam_step_rows)
    normal_consistency_loss   2DGS's normal-consistency regulariser over fused.rasterize_normals' maps and
                              fused.depth_to_normal (plain torch over the kernel's output: not a hot path)
    accumulate_grad_stats     trainer.py:378-385 (densification statistics) in one launch, without
                              the boolean-mask index_put and its host sync

Anything the HIP kernel does not cover (amsgrad, weight decay, maximize, capturable, sparse or
non-fp32 / non-device tensors) is handed to torch.optim.Adam.step itself.
"""
import ctypes

import torch
from torch.optim.adam import adam as _torch_adam   # the functional form (torch.optim.adam itself is not an attribute)

from . import _hip

_MAX_TENSORS = 8   # per launch (csrc/train_ops.hip)


class Adam(torch.optim.Adam):
    def _hip_ok(self, group):
        if group["amsgrad"] or group["weight_decay"] != 0 or group["maximize"] or group.get("capturable", False):
            return False
        if group.get("differentiable", False):
            return False
        for p in group["params"]:
            if p.grad is None:
                continue
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and not p.grad.is_sparse
                    and p.grad.dtype == torch.float32):
                return False
        return True

    @torch.no_grad()
    def step(self, closure=None):
        if not all(self._hip_ok(g) for g in self.param_groups):
            return super().step(closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:   # torch/optim/adam.py _init_group
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["step"] += 1
                grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                work.append((p, grad, state["exp_avg"], state["exp_avg_sq"], float(group["lr"]),
                             int(state["step"]), beta1, beta2, group["eps"]))
        stream = _hip.current_stream()
        i = 0
        while i < len(work):
            # one launch per run of tensors that share (beta1, beta2, eps): all of them, normally
            j = i
            while j < len(work) and j - i < _MAX_TENSORS and work[j][6:] == work[i][6:]:
                j += 1
            chunk = work[i:j]
            n = len(chunk)
            ptrs = lambda k: (ctypes.c_void_p * n)(*[t[k].data_ptr() for t in chunk])
            _hip.call("gs_adam_step", n, ptrs(0), ptrs(1), ptrs(2), ptrs(3),
                      (ctypes.c_int64 * n)(*[t[0].numel() for t in chunk]),
                      (ctypes.c_double * n)(*[t[4] for t in chunk]), (ctypes.c_int64 * n)(*[t[5] for t in chunk]),
                      chunk[0][6], chunk[0][7], chunk[0][8], stream)
            i = j
        # the kernel wrote through raw pointers: bump the version counters like an in-place torch op would,
        # so that autograd's saved-tensor check still catches a backward over stale parameters
        for p, _, m, v, *_ in work:
            torch.autograd.graph.increment_version(p)
            torch.autograd.graph.increment_version(m)
            torch.autograd.graph.increment_version(v)
        return loss


class SelectiveAdam(Adam):
    """train_ops.Adam (same constructor, param_groups and state layout, so a DensityController's parameter surgery
    works on it unchanged) whose step can leave alone the Gaussians a frame did not see:

        opt = SelectiveAdam(param_groups)
        image, culling_mask, uv = fused.rasterize(...)
        loss.backward()
        opt.step(culling_mask=culling_mask)        # keyword only; None -> Adam.step

    culling_mask: [N] bool, True = skip, as rasterize returns it; every parameter with a gradient has shape[0] == N.

      rows with culling_mask[r] == False   p[r], exp_avg[r], exp_avg_sq[r] take exactly the update Adam.step applies in
                                           the same step (bias correction from the tensor's own state["step"] after its
                                           increment): bit for bit a dense step restricted to those rows
      rows with culling_mask[r] == True    every bit of p[r], exp_avg[r], exp_avg_sq[r] stays (no moment decay, no drift
                                           on stale momentum; NaN payloads and infinities included); the gradient is
                                           not read there and need not be zero
      state["step"]                        advances by one for every parameter that has a .grad, whatever the mask
                                           says (an all-True mask included): the count is global, not per row

    step(culling_mask=None) is Adam.step, with its results.  With a mask, amsgrad / weight decay / maximize /
    capturable / differentiable in any group raise RuntimeError; a mask that is not a 1-D bool tensor on the
    parameters' device, or a parameter whose shape[0] differs from the mask's, raises ValueError before any state
    is touched.  fp32 contiguous device tensors go through one gs_adam_step_rows launch per run of at most 8 tensors
    that share (betas, eps); anything else (CPU, other dtypes, non-contiguous) through torch's functional Adam on the
    gathered visible rows, which are scattered back -- culled rows are not written at all.

    A caller that accumulates gradients over several frames before one step passes the AND of their culling masks
    (a row is skipped only if no frame saw it).  On an owner-sliced multi-GPU job, where a rank steps only its own
    rows, the caller passes the slice of the mask that matches those rows."""

    @torch.no_grad()
    def step(self, closure=None, *, culling_mask=None):
        if culling_mask is None:
            return super().step(closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        mask = culling_mask
        if not (torch.is_tensor(mask) and mask.dtype == torch.bool and mask.dim() == 1):
            what = f"{tuple(mask.shape)} {mask.dtype}" if torch.is_tensor(mask) else type(mask).__name__
            raise ValueError(f"SelectiveAdam: culling_mask must be a 1-D bool tensor, got {what}")
        for gi, group in enumerate(self.param_groups):
            for pi, p in enumerate(group["params"]):
                if p.grad is None:
                    continue
                if p.device != mask.device:
                    raise ValueError(f"SelectiveAdam: culling_mask is on {mask.device}, parameter {pi} of group {gi} "
                                     f"on {p.device}")
                if p.dim() == 0 or p.shape[0] != mask.shape[0]:
                    raise ValueError(f"SelectiveAdam: parameter {pi} of group {gi} has shape {tuple(p.shape)}, "
                                     f"culling_mask {mask.shape[0]} rows")
        for gi, group in enumerate(self.param_groups):
            for name in ("amsgrad", "weight_decay", "maximize", "capturable", "differentiable"):
                if group.get(name, False):
                    raise RuntimeError(f"SelectiveAdam: {name} in param group {gi} is not supported with a culling_mask")
        N = mask.shape[0]
        mask = mask.contiguous()
        visible = None   # row indices for the torch path, made on first use
        work = []
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:   # torch/optim/adam.py _init_group
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["step"] += 1
                if p.numel() == 0:
                    continue
                m, v = state["exp_avg"], state["exp_avg_sq"]
                if (p.is_cuda and not p.grad.is_sparse
                        and all(t.dtype == torch.float32 and t.is_contiguous() for t in (p, m, v))
                        and p.grad.dtype == torch.float32):
                    grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                    work.append((p, grad, m, v, float(group["lr"]), int(state["step"]), beta1, beta2, group["eps"]))
                    continue
                if visible is None:
                    visible = (~mask).nonzero().squeeze(1)
                if visible.numel() == 0:
                    continue
                grad = p.grad.to_dense() if p.grad.is_sparse else p.grad
                rows = [t.index_select(0, visible) for t in (p, grad, m, v)]
                # _single_tensor_adam increments the step it is given
                _torch_adam([rows[0]], [rows[1]], [rows[2]], [rows[3]], [], [state["step"] - 1], foreach=False,
                            amsgrad=False, beta1=beta1, beta2=beta2, lr=group["lr"], weight_decay=0, eps=group["eps"],
                            maximize=False)
                p.index_copy_(0, visible, rows[0])
                m.index_copy_(0, visible, rows[2])
                v.index_copy_(0, visible, rows[3])
        if work:
            stream = _hip.current_stream()
        i = 0
        while i < len(work):
            j = i
            while j < len(work) and j - i < _MAX_TENSORS and work[j][6:] == work[i][6:]:
                j += 1
            chunk = work[i:j]
            n = len(chunk)
            ptrs = lambda k: (ctypes.c_void_p * n)(*[t[k].data_ptr() for t in chunk])
            _hip.call("gs_adam_step_rows", n, ptrs(0), ptrs(1), ptrs(2), ptrs(3),
                      (ctypes.c_int64 * n)(*[t[0].numel() for t in chunk]),
                      (ctypes.c_int64 * n)(*[t[0].numel() // N for t in chunk]), mask.data_ptr(), N,
                      (ctypes.c_double * n)(*[t[4] for t in chunk]), (ctypes.c_int64 * n)(*[t[5] for t in chunk]),
                      chunk[0][6], chunk[0][7], chunk[0][8], stream)
            i = j
        for p, _, m, v, *_ in work:   # as Adam.step: the kernel wrote through raw pointers
            torch.autograd.graph.increment_version(p)
            torch.autograd.graph.increment_version(m)
            torch.autograd.graph.increment_version(v)
        return loss


_FUSED_NAMES = ("quaternion", "scale", "opacity", "rgb", "sh")   # stepped in the backward; xyz stays with step()
_GROUP_ORDER = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")   # densify.GROUP_ORDER (optimizer_manager.py:15-42)


class _FusedPlan:
    """What one frame's backward needs to step the five tensors: handed to fused.rasterize, asked by the
    per-Gaussian backward node (Python or native) at backward time."""

    def __init__(self, opt, items):
        self.opt = opt
        self.items = items   # [(name, parameter, param group)] in _FUSED_NAMES order, without sh when there is none

    def begin(self):
        """-> ([(param, exp_avg, exp_avg_sq, lr, step) x 5 (sh: None without SH)], beta1, beta2, eps), with the
        hyper-parameters as the groups hold them NOW and every state["step"] advanced by one"""
        opt = self.opt
        shared = None
        for name, p, group in self.items:
            if not (opt._group_ok(group) and len(group["params"]) == 1 and group["params"][0] is p):
                raise RuntimeError(f"FusedRasterAdam: the param group of '{name}' changed between rasterize() and backward()")
            key = (tuple(group["betas"]), group["eps"])
            shared = key if shared is None else shared
            if key != shared:
                raise RuntimeError("FusedRasterAdam: betas / eps of the groups differ at backward()")
        rows = []
        for name, p, group in self.items:
            state = opt.state[p]
            if len(state) == 0:   # torch/optim/adam.py _init_group
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["step"] += 1
            rows.append((p, state["exp_avg"], state["exp_avg_sq"], float(group["lr"]), int(state["step"])))
            opt._stepped_in_backward[id(p)] = (name, p)
        rows += [None] * (len(_FUSED_NAMES) - len(rows))
        (beta1, beta2), eps = shared
        return rows, float(beta1), float(beta2), float(eps)


class FusedRasterAdam(Adam):
    """train_ops.Adam (same constructor, param_groups and state layout) with the optimizer step of five of the six
    parameter tensors folded into the frame's backward:

        opt = FusedRasterAdam(param_groups)      # one group per tensor: xyz, quaternion, scale, opacity, rgb[, sh]
        image, culling_mask, uv = opt.rasterize(gaussians, camera_T_world, camera, near_thresh, far_thresh,
                                                cull_mask_padding, mh_dist, use_sh_precompute, background_rgb)
        loss.backward()     # quaternion / scale / opacity / rgb / sh are stepped inside the backward
        opt.step()          # steps what the backward did not: xyz (and everything on a fallback frame)

    rasterize() has fused.rasterize's (image, culling_mask, uv) contract; uv.retain_grad() / uv.grad and
    gaussians.xyz.grad work as they do there.  A parameter stepped in the backward comes out with .grad None, its
    state["step"] advanced by one; lr / betas / eps are read from its group at backward time.  step() skips it as
    Adam.step skips any parameter without a gradient -- and raises RuntimeError if it nevertheless has a .grad
    (another consumer in the graph, e.g. a regulariser on scale): stepping it again would apply two steps.

    The parameters are looked up per call: group i of param_groups in the reference's order (densify.GROUP_ORDER)
    must hold exactly the tensor of `gaussians`, so a DensityController may swap them between iterations.

    The fused step is taken only when all of this holds -- otherwise rasterize() IS fused.rasterize and step() IS
    Adam.step, with today's results: fp32 contiguous device leaf tensors that require grad, grad mode on,
    use_sh_precompute or no SH, no amsgrad / weight decay / maximize / capturable / differentiable in the five
    groups, which all share betas and eps.

    Limits: the single-GPU frame only (no tile_rows, hooks or `sharded`).  The step modifies quaternion and scale,
    which the frame saved for its backward: a second backward over a retained graph fails autograd's in-place
    check.  Every backward is a step: accumulating gradients over several frames before one step() is not what
    this mode does (use Adam for that)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._stepped_in_backward = {}
        self.last_fallback_reason = None   # why the latest rasterize() did not take the fused step (None: it did)

    @staticmethod
    def _group_ok(group):
        return not (group["amsgrad"] or group["weight_decay"] != 0 or group["maximize"]
                    or group.get("capturable", False) or group.get("differentiable", False))

    def fused_decision(self, gaussians, use_sh_precompute=True):
        """-> (plan, None) when the frame's backward can take the fused step, else (None, why not).  Looks at the
        param groups first and then at tensor metadata only: nothing here touches the device."""
        g = gaussians
        if not torch.is_grad_enabled():
            return None, "grad mode is off"
        if g.sh is not None and not use_sh_precompute:
            return None, "per-pixel SH colour (use_sh_precompute=False)"
        names = [k for k in _FUSED_NAMES if getattr(g, k) is not None]
        if names[:4] != list(_FUSED_NAMES[:4]):
            return None, "a parameter tensor is missing"
        shared = None
        for name in names:
            i = _GROUP_ORDER.index(name)
            if i >= len(self.param_groups):
                return None, f"no param group for '{name}'"
            group = self.param_groups[i]
            if not (len(group["params"]) == 1 and group["params"][0] is getattr(g, name)):
                return None, f"param group {i} does not hold exactly the '{name}' tensor of the Gaussians"
            for opt_name in ("amsgrad", "weight_decay", "maximize", "capturable", "differentiable"):
                if group.get(opt_name, False):
                    return None, f"{opt_name} in the group of '{name}'"
            key = (tuple(group["betas"]), group["eps"])
            shared = key if shared is None else shared
            if key != shared:
                return None, "the groups do not share betas and eps"
        if not (g.xyz.is_cuda and g.xyz.dtype == torch.float32 and g.xyz.shape[0] > 0):
            return None, "not fp32 device tensors"
        items = []
        for name in names:
            p = getattr(g, name)
            if not (p.is_cuda and p.device == g.xyz.device and p.dtype == torch.float32 and p.is_contiguous()
                    and p.shape[0] == g.xyz.shape[0]):
                return None, f"'{name}' is not a contiguous fp32 tensor on the device of xyz"
            if not (p.requires_grad and p.is_leaf):
                return None, f"'{name}' is not a leaf that requires grad"
            state = self.state.get(p)
            if state:
                for k in ("exp_avg", "exp_avg_sq"):
                    t = state.get(k)
                    if not (torch.is_tensor(t) and t.is_cuda and t.device == p.device and t.dtype == torch.float32
                            and t.is_contiguous() and t.shape == p.shape):
                        return None, f"the optimizer state of '{name}' is not in the kernel's layout"
                if "step" not in state:
                    return None, f"the optimizer state of '{name}' has no step count"
            items.append((name, p, self.param_groups[_GROUP_ORDER.index(name)]))
        return _FusedPlan(self, items), None

    def fused_plan(self, gaussians, use_sh_precompute=True):
        plan, self.last_fallback_reason = self.fused_decision(gaussians, use_sh_precompute)
        return plan

    def rasterize(self, gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                  use_sh_precompute, background_rgb):
        from . import fused

        plan = self.fused_plan(gaussians, use_sh_precompute)
        return fused.rasterize(gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                               use_sh_precompute, background_rgb, adam_plan=plan)

    def step(self, closure=None):
        stepped, self._stepped_in_backward = self._stepped_in_backward, {}
        for name, p in stepped.values():
            if p.grad is not None:
                raise RuntimeError(f"FusedRasterAdam: '{name}' was stepped inside the backward but has a .grad at step() "
                                   "(another consumer of it in the graph?): stepping it again would apply two steps")
        return super().step(closure)


def accumulate_grad_stats(uv_grad, culling_mask, xyz_grad, camera, uv_grad_accum, xyz_grad_accum, grad_accum_count):
    """trainer.py:378-385:

        uv_grad[:, 0] *= K[0, 0]; uv_grad[:, 1] *= K[1, 1]
        uv_grad_accum[~culling_mask] += |uv_grad|; xyz_grad_accum += |xyz.grad|
        grad_accum_count += (~culling_mask).int()

    uv_grad: [V, 2] (any row stride, e.g. the view of the fused path's slab); it is NOT modified.  The uv_absgrad of
    fused.rasterize(..., absgrad=True) goes here in place of uv.grad unchanged: it is already >= 0, the same scaling
    and sums apply.
    The focal lengths are read from camera.K on the device (no host sync)."""
    N = culling_mask.shape[0]
    keep = ~culling_mask
    rank = torch.where(keep, torch.cumsum(keep, 0, dtype=torch.int32) - 1,
                       torch.full((), -1, dtype=torch.int32, device=keep.device)).to(torch.int32)
    if uv_grad.stride(1) != 1:
        uv_grad = uv_grad.contiguous()
    K = camera.K if (camera.K.dtype == torch.float32 and camera.K.is_contiguous()) else \
        camera.K.to(torch.float32).contiguous()
    p = _hip.ptr
    _hip.call("gs_accumulate_grad_stats", p(uv_grad), uv_grad.stride(0) if uv_grad.shape[0] else 2, p(rank),
              p(xyz_grad), p(K), N, p(uv_grad_accum), p(xyz_grad_accum), p(grad_accum_count), _hip.current_stream())


class _SsimL1Loss(torch.autograd.Function):
    """value and d loss / d image from one launch; backward scales the stored gradient"""

    @staticmethod
    def forward(ctx, image, target, ssim_frac):
        H, W = image.shape[0], image.shape[1]
        dev = image.device
        ws = torch.empty(_hip.lib().gs_ssim_l1_workspace_bytes(H, W) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        need_grad = image.requires_grad
        grad = torch.empty_like(image) if need_grad else None
        p = _hip.ptr
        _hip.call("gs_ssim_l1_loss", p(image), p(target), H, W, ssim_frac, p(ws), p(out), p(grad), _hip.current_stream())
        ctx.grad = grad
        ctx.mark_non_differentiable(out)
        return out[0], out

    @staticmethod
    def backward(ctx, g_loss, _unused):
        if ctx.grad is None or g_loss is None:
            return None, None, None
        return ctx.grad * g_loss, None, None


def ssim_l1_loss(image, target, ssim_frac=0.2, return_terms=False):
    """The reference's training loss (trainer.py:363-374):

        (1 - ssim_frac) * l1_loss(image, target) + ssim_frac * (1 - SSIM(image, target))

    image, target: [H, W, 3] fp32 device tensors (the rasterizer's layout; the reference permutes
    them to NCHW for torchmetrics).  -> loss (0-d, differentiable w.r.t. image); with
    return_terms=True also the detached (loss, l1, ssim, mse) tensor (psnr = -10 log10(mse),
    trainer.py:366-367)."""
    if not (image.is_cuda and image.dtype == torch.float32 and image.dim() == 3 and image.shape[2] == 3):
        raise RuntimeError("ssim_l1_loss takes [H, W, 3] float32 device tensors")
    if target.shape != image.shape or target.dtype != image.dtype or target.device != image.device:
        raise RuntimeError("ssim_l1_loss: target must match image")
    loss, terms = _SsimL1Loss.apply(image.contiguous(), target.contiguous(), ssim_frac)
    return (loss, terms) if return_terms else loss


def normal_consistency_loss(normal_map, depth, alpha, camera, camera_model="pinhole", min_alpha=0.0, depth_alpha=None):
    """The normal-consistency regulariser of 2DGS over the maps of fused.rasterize_normals:

        mean over the valid pixels of  alpha.detach() - sum_c normal_map[..., c] * n_d[..., c]

    with n_d = fused.depth_to_normal(depth, depth_alpha, camera, camera_model, min_alpha) and a pixel valid where n_d exists:
    2DGS's 1 - N . (alpha n_d) for its unnormalised N, restricted to the pixels that have a depth normal.  -> a 0-d
    tensor, differentiable in normal_map, depth and alpha; a frame without a valid pixel gives a zero that still carries
    the graph.  Composed in PyTorch over the kernel's output: a handful of elementwise launches and two reductions per
    frame, not a hot path; no host read.
    depth_alpha: the map depth is divided by and validated against inside depth_to_normal.  None (the default) is alpha:
    depth is then the unnormalised sum w z, and the result has the bits it had before the keyword existed.  With the
    median depth of fused.rasterize_median_depth, which is a depth already, pass depth=median_depth and
    depth_alpha=(median_index >= 0).float(); alpha stays the frame's accumulated opacity in the loss term."""
    from . import fused
    if not (torch.is_tensor(normal_map) and normal_map.dim() == 3 and normal_map.shape[2] == 3
            and normal_map.shape[:2] == depth.shape):
        raise RuntimeError("normal_consistency_loss: normal_map must be [H, W, 3] over depth's [H, W]")
    n_d = fused.depth_to_normal(depth, alpha if depth_alpha is None else depth_alpha, camera, camera_model, min_alpha)
    valid = (n_d.detach() != 0).any(dim=2)
    per_pixel = alpha.detach() - (normal_map * n_d).sum(dim=2)
    return torch.where(valid, per_pixel, torch.zeros_like(per_pixel)).sum() / valid.sum().clamp(min=1)
