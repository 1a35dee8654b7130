"""Adaptive density control on the device (reference: splat_py/trainer.py:50-295 and
splat_py/optimizer_manager.py:44-172).

    ctrl = DensityController(gaussians, optimizer, DensifyConfig())
    ... per iteration:  ctrl.accumulate(uv.grad, culling_mask, camera)            # trainer.py:378-385
    ... every adaptive_control_interval iterations:  ctrl.adaptive_density_control(it)   # :208-295
    ... ctrl.reset_opacity() (:68-75), ctrl.add_sh_band() (:77-112)

The reference performs one density-control step as ~60 PyTorch calls with 10+ host synchronisations
(boolean-mask gathers of six parameter tensors and twelve optimizer-state tensors, per operation, plus
`.item()` / `.cpu().numpy()` prints).  Here the DECISIONS are formed with the reference's own expressions
on the device (same tensors, same torch.quantile -- so the masks are the reference's bit for bit), the
masks become destination indices with prefix sums, and ONE HIP launch (gs_densify_move,
csrc/densify.hip) reads every old row once and writes every new row once for all parameters and their
Adam moments.  One host read per step (the three counts that size the new tensors).

`optimizer` is the torch.optim.Adam (or gaussian_splatting_amd.train_ops.Adam) the reference's
OptimizerManager builds: one param group per tensor in the order xyz, quaternion, scale, opacity, rgb[, sh]
(optimizer_manager.py:15-42).  The controller swaps the parameters inside those groups and re-keys the state
exactly as OptimizerManager does, so `optimizer.step()` keeps working across steps.
"""
import ctypes
import math
from dataclasses import dataclass

import torch

from . import _hip
from .train_ops import accumulate_grad_stats

GROUP_ORDER = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")   # optimizer_manager.py:15-42
_KIND = {"xyz": 1, "scale": 2, "quaternion": 3}


@dataclass
class DensifyConfig:
    """the density-control fields of the reference's SplatConfig with its defaults (config.py:100-157)"""
    reset_opacity_value: float = 0.20
    max_sh_band: int = 3
    use_split: bool = True
    use_clone: bool = True
    use_delete: bool = True
    adaptive_control_start: int = 750
    adaptive_control_end: int = 6500
    adaptive_control_interval: int = 100
    max_gaussians: int = 4250000
    delete_opacity_threshold: float = 0.1
    clone_scale_threshold: float = 0.01
    use_fractional_densification: bool = True
    use_adaptive_fractional_densification: bool = True
    uv_grad_percentile: float = 0.96
    scale_norm_percentile: float = 0.99
    uv_grad_threshold: float = 0.0002
    split_scale_factor: float = 1.6
    num_split_samples: int = 2
    # learning rate of the SH group add_sh_band creates when there is none yet: base_lr * sh_lr_multiplier
    # (config.py:80,93 -> optimizer_manager.py:60-63)
    sh_lr: float = 0.002 * 0.1


def inverse_sigmoid(x):   # utils.py:11-15
    return math.log(x / (1.0 - x))


_p = _hip.ptr


class DensityController:
    def __init__(self, gaussians, optimizer, config=None):
        self.gaussians = gaussians
        self.optimizer = optimizer
        self.config = config if config is not None else DensifyConfig()
        self.reset_grad_accum()
        self.last_info = {}

    # ---- accumulators (trainer.py:50-66, 378-385) ---------------------------------------------------------
    def reset_grad_accum(self):
        xyz = self.gaussians.xyz
        n, kw = xyz.shape[0], dict(dtype=xyz.dtype, device=xyz.device)
        self.uv_grad_accum = torch.zeros(n, 2, **kw)
        self.xyz_grad_accum = torch.zeros(n, 3, **kw)
        self.grad_accum_count = torch.zeros(n, dtype=torch.int32, device=xyz.device)

    def accumulate(self, uv_grad, culling_mask, camera):
        """the densification statistics of one training iteration (call after backward).
        uv_grad: any [V, 2] tensor of the frame's visible Gaussians -- uv.grad, or in its place the uv_absgrad of
        fused.rasterize(..., absgrad=True) (AbsGS: the per-pixel magnitudes, which do not cancel for a large Gaussian
        with detail on both sides of its centre).  Either way |K-scaled value| is accumulated; a fixed
        uv_grad_threshold has to be raised for absgrad, the percentile mode adapts by itself."""
        accumulate_grad_stats(uv_grad, culling_mask, self.gaussians.xyz.grad, camera, self.uv_grad_accum,
                              self.xyz_grad_accum, self.grad_accum_count)

    # ---- optimizer plumbing (optimizer_manager.py:44-172) ---------------------------------------------------
    def _names(self):
        return [k for k in GROUP_ORDER if getattr(self.gaussians, k) is not None]

    def _group(self, name):
        return self.optimizer.param_groups[GROUP_ORDER.index(name)]

    def _state(self, name):
        group = self._group(name)
        return self.optimizer.state.get(group["params"][0], None) if group["params"] else None

    def _swap(self, name, new_tensor, exp_avg=None, exp_avg_sq=None, restart=False):
        """puts new_tensor (as a Parameter) into the Gaussians struct and the optimizer group `name`, moving
        the parameter's state entry to the new key with the given moments (None: keep the old ones).
        restart: Adam's step count of the entry goes back to 0 as well -- the reference stores the reset state
        under the integer keys optimizer.state[3] / [5] (optimizer_manager.py:57,76), which orphans it, so its
        optimizer re-initialises the new parameter at the next step(): zero moments AND step 0 (bias
        correction restarts; with the old step count the first updates would be ~3.2x smaller)"""
        group = self._group(name)
        old = group["params"][0]
        state = self.optimizer.state.pop(old, None)
        param = torch.nn.Parameter(new_tensor)
        group["params"] = [param]
        if state:
            if exp_avg is not None:
                state["exp_avg"], state["exp_avg_sq"] = exp_avg, exp_avg_sq
            if restart and "step" in state:
                state["step"] = torch.zeros_like(state["step"]) if torch.is_tensor(state["step"]) else 0
            self.optimizer.state[param] = state
        setattr(self.gaussians, name, param)

    # ---- trainer.py:68-75 ------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset_opacity(self):
        old = self.gaussians.opacity
        st = self._state("opacity")
        zeros = (torch.zeros_like(old), torch.zeros_like(old)) if st else (None, None)
        self._swap("opacity", torch.ones_like(old) * inverse_sigmoid(self.config.reset_opacity_value), *zeros,
                   restart=True)
        self.reset_grad_accum()

    # ---- trainer.py:77-112 -----------------------------------------------------------------------------------
    @torch.no_grad()
    def add_sh_band(self):
        g, cfg = self.gaussians, self.config
        n = g.xyz.shape[0]
        if cfg.max_sh_band == 0:
            return
        if g.sh is None:
            g.sh = torch.nn.Parameter(torch.zeros(n, 3, 3, dtype=g.rgb.dtype, device=g.rgb.device))
            self.optimizer.add_param_group({"params": g.sh, "lr": cfg.sh_lr})
            return
        width = g.sh.shape[2]
        grow = {3: 8, 8: 15}.get(width)
        if grow is None or cfg.max_sh_band <= {3: 1, 8: 2}[width]:
            return
        new_sh = torch.zeros(n, 3, grow, dtype=g.rgb.dtype, device=g.rgb.device)
        new_sh[:, :, :width] = g.sh.detach()
        st = self._state("sh")
        zeros = (torch.zeros_like(new_sh), torch.zeros_like(new_sh)) if st else (None, None)
        self._swap("sh", new_sh, *zeros, restart=True)

    # ---- trainer.py:208-295 ----------------------------------------------------------------------------------
    @torch.no_grad()
    def adaptive_density_control(self, it, rand=None):
        """One density-control step.  rand(n) -> [n, 3] uniform samples for the split (default:
        torch.rand on the device, trainer.py:176).  -> dict with the counts of the step."""
        g, cfg = self.gaussians, self.config
        info = self.last_info = {}
        if not (cfg.use_delete or cfg.use_clone or cfg.use_split):
            return info
        dev = g.xyz.device
        N0 = g.xyz.shape[0]
        i32 = dict(dtype=torch.int32, device=dev)

        # Step 1: the delete decision (trainer.py:213-230), on all N0 rows
        keep = (g.opacity.detach() > inverse_sigmoid(cfg.delete_opacity_threshold)).squeeze(1)
        keep &= ~(self.grad_accum_count == 0)
        keep &= ~(torch.norm(self.uv_grad_accum, dim=1) == 0.0)
        if not cfg.use_delete:
            keep = torch.ones_like(keep)
        # Step 2 works on the survivors: the same expressions on the compacted statistics (the
        # per-row values do not change by compaction; torch.quantile sees exactly the survivors)
        cnt = self.grad_accum_count[keep].unsqueeze(1).float()
        uv_norm = torch.norm(self.uv_grad_accum[keep] / cnt, dim=1)
        scale_max = g.scale.detach()[keep].exp().max(dim=-1).values
        N1 = uv_norm.shape[0]
        if N1 > cfg.max_gaussians:   # trainer.py:232-235: delete only
            clone_s = split_s = torch.zeros(N1, dtype=torch.bool, device=dev)
            split_c = clone_s
            info["skipped"] = True
        else:
            if cfg.use_adaptive_fractional_densification:
                factor = (float(cfg.adaptive_control_end - it)
                          / float(cfg.adaptive_control_end - cfg.adaptive_control_start) * 2.0)
            else:
                factor = 1.0
            if cfg.use_fractional_densification:
                f = factor if cfg.use_adaptive_fractional_densification else 1.0
                uv_split_val = torch.quantile(uv_norm, 1.0 - (1.0 - cfg.uv_grad_percentile) * f) if N1 else 0.0
            else:
                uv_split_val = cfg.uv_grad_threshold
            densify = uv_norm > uv_split_val
            clone_s = densify & (scale_max <= cfg.clone_scale_threshold)
            if not cfg.use_clone:
                clone_s = torch.zeros_like(clone_s)
            # the split decision over [survivors, clones] (trainer.py:268-284): a clone carries its source's
            # densify flag and scale_max, so its decision is its source's, evaluated with the quantile of
            # the concatenated scale_max
            scale_all = torch.cat([scale_max, scale_max[clone_s]], dim=0)
            if scale_all.numel():
                scale_split = torch.quantile(scale_all, 1.0 - (1.0 - cfg.scale_norm_percentile) * factor)
                split_s = (densify & (scale_max > cfg.clone_scale_threshold)) | (scale_max > scale_split)
            else:
                split_s = torch.zeros_like(clone_s)
            if not cfg.use_split:
                split_s = torch.zeros_like(split_s)
            split_c = split_s & clone_s

        # destination indices (survivor space), then scattered back to the N0 source rows
        stay_s = ~split_s
        stay_c = clone_s & ~split_c
        a_self = torch.cumsum(stay_s, 0, dtype=torch.int32) - 1
        n_a_self = int(0)
        counts = torch.stack([stay_s.sum(), stay_c.sum(), split_s.sum(), split_c.sum()]).tolist()   # the host read
        n_a_self, n_a_clone, p_self, p_clone = counts
        a_clone = n_a_self + torch.cumsum(stay_c, 0, dtype=torch.int32) - 1
        r_self = torch.cumsum(split_s, 0, dtype=torch.int32) - 1
        r_clone = p_self + torch.cumsum(split_c, 0, dtype=torch.int32) - 1
        minus = torch.full((), -1, **i32)
        src_rows = torch.nonzero(keep, as_tuple=False).flatten()

        def scatter(values, mask):
            out = torch.full((N0,), -1, **i32)
            out[src_rows] = torch.where(mask, values.to(torch.int32), minus)
            return out

        dst_self, dst_clone = scatter(a_self, stay_s), scatter(a_clone, stay_c)
        spl_self, spl_clone = scatter(r_self, split_s), scatter(r_clone, split_c)
        P = p_self + p_clone
        samples = cfg.num_split_samples
        sample_base = n_a_self + n_a_clone
        n_new = sample_base + P * samples
        info.update(deleted=N0 - N1, cloned=int(n_a_clone + p_clone), split=int(P), n_before=N0, n_after=int(n_new))
        random_samples = (rand(P * samples) if rand is not None else torch.rand(P * samples, 3, device=dev)) \
            if P else torch.zeros(0, 3, device=dev)

        names = self._names()
        src, dst, src_m, dst_m, src_v, dst_v = [], [], [], [], [], []
        for k in names:
            t = getattr(g, k).detach().contiguous()
            st = self._state(k)
            has = bool(st) and "exp_avg" in st
            src.append(t)
            dst.append(torch.empty((n_new,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev))
            src_m.append(st["exp_avg"].contiguous() if has else None)
            src_v.append(st["exp_avg_sq"].contiguous() if has else None)
            dst_m.append(torch.empty_like(dst[-1]) if has else None)
            dst_v.append(torch.empty_like(dst[-1]) if has else None)
        n = len(names)
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])
        widths = (ctypes.c_int32 * n)(*[int(t[0].numel()) if t.shape[0] else int(math.prod(t.shape[1:])) for t in src])
        kinds = (ctypes.c_int32 * n)(*[_KIND.get(k, 0) for k in names])
        xyz_s, scale_s, quat_s = (src[names.index(k)] for k in ("xyz", "scale", "quaternion"))
        _hip.call("gs_densify_move", n, arr(src), arr(dst), arr(src_m), arr(dst_m), arr(src_v), arr(dst_v), widths,
                  kinds, N0, _p(dst_self), _p(dst_clone), _p(spl_self), _p(spl_clone), _p(xyz_s), _p(scale_s),
                  _p(quat_s), _p(self.xyz_grad_accum), _p(self.grad_accum_count), _p(random_samples.contiguous()),
                  int(P), int(samples), int(sample_base), cfg.split_scale_factor, _hip.current_stream())
        for k, d, m, v in zip(names, dst, dst_m, dst_v):
            self._swap(k, d, m, v)
        self.reset_grad_accum()
        return info

    # ---- pruning (no reference counterpart) -------------------------------------------------------------------
    @torch.no_grad()
    def prune(self, keep):
        """Deletes the Gaussians whose row of keep ([N] bool on the Gaussians' device) is False: the delete of
        adaptive_density_control on its own, with the caller's decision.  One gs_densify_move with destinations only
        (dst_self = the prefix-sum index of the kept rows, no clone, no split) moves every parameter tensor and its
        Adam moments; the step counts are kept, the gradient accumulators reset, the optimizer groups re-keyed.  One
        host read (the new count).  -> {"deleted", "n_before", "n_after"}"""
        g = self.gaussians
        dev = g.xyz.device
        N0 = g.xyz.shape[0]
        if not (torch.is_tensor(keep) and keep.dtype == torch.bool and tuple(keep.shape) == (N0,) and keep.device == dev):
            raise RuntimeError(f"prune: keep must be a [{N0}] bool tensor on {dev}")
        dst_pos = torch.cumsum(keep, 0, dtype=torch.int32) - 1
        n_new = int(dst_pos[-1].item()) + 1 if N0 else 0   # the host read
        info = self.last_info = dict(deleted=N0 - n_new, n_before=N0, n_after=n_new)
        if n_new == N0:
            return info
        minus = torch.full((N0,), -1, dtype=torch.int32, device=dev)
        dst_self = torch.where(keep, dst_pos, minus)
        names = self._names()
        src, dst, src_m, dst_m, src_v, dst_v = [], [], [], [], [], []
        for k in names:
            t = getattr(g, k).detach().contiguous()
            st = self._state(k)
            has = bool(st) and "exp_avg" in st
            src.append(t)
            dst.append(torch.empty((n_new,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev))
            src_m.append(st["exp_avg"].contiguous() if has else None)
            src_v.append(st["exp_avg_sq"].contiguous() if has else None)
            dst_m.append(torch.empty_like(dst[-1]) if has else None)
            dst_v.append(torch.empty_like(dst[-1]) if has else None)
        n = len(names)
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])
        widths = (ctypes.c_int32 * n)(*[int(math.prod(t.shape[1:])) for t in src])
        kinds = (ctypes.c_int32 * n)(*[_KIND.get(k, 0) for k in names])
        xyz_s, scale_s, quat_s = (src[names.index(k)] for k in ("xyz", "scale", "quaternion"))
        no_samples = torch.zeros(1, 3, device=dev)   # (n_split == 0: never read)
        _hip.call("gs_densify_move", n, arr(src), arr(dst), arr(src_m), arr(dst_m), arr(src_v), arr(dst_v), widths,
                  kinds, N0, _p(dst_self), _p(minus), _p(minus), _p(minus), _p(xyz_s), _p(scale_s), _p(quat_s),
                  _p(self.xyz_grad_accum), _p(self.grad_accum_count), _p(no_samples), 0, 0, n_new, 1.0,
                  _hip.current_stream())
        for k, d, m, v in zip(names, dst, dst_m, dst_v):
            self._swap(k, d, m, v)
        self.reset_grad_accum()
        return info

    def prune_by_contribution(self, stats, min_weight_max):
        """prune() by RadSplat's criterion on a fused.ContributionStats swept over the training views: keeps the
        Gaussians whose largest blending weight at any pixel reached min_weight_max.  With min_weight_max = 0 only the
        Gaussians that contributed to no pixel of any view (pixel_count == 0) go."""
        n = self.gaussians.xyz.shape[0]
        if stats.weight_max.shape[0] != n or stats.pixel_count.shape[0] != n:
            raise RuntimeError(f"prune_by_contribution: the statistics are of {stats.weight_max.shape[0]} Gaussians, the set "
                               f"has {n} (sweep the views again after N changed)")
        # (a positive threshold implies pixel_count > 0; at 0 the count alone decides)
        return self.prune((stats.weight_max >= min_weight_max) & (stats.pixel_count > 0))


# ---- MCMC densification (no reference counterpart) ------------------------------------------------------
@dataclass
class MCMCConfig:
    """3DGS-MCMC ("3D Gaussian Splatting as Markov Chain Monte Carlo") with the defaults in wide use"""
    cap_max: int = 1_000_000        # the budget: add_new never grows the set beyond it
    min_opacity: float = 0.005      # a Gaussian at or below it is dead
    grow_factor: float = 1.05       # growth per refinement step
    noise_lr: float = 5e5           # position noise = noise_lr * xyz_lr * gate(opacity) * Sigma_world * N(0, 1)
    gate_k: float = 100.0
    gate_x0: float = 0.995
    refine_start: int = 500
    refine_stop: int = 25_000
    refine_every: int = 100
    opacity_reg: float = 0.01
    scale_reg: float = 0.01


_MCMC_KIND = {"scale": 2, "opacity": 4}   # gs_mcmc_relocate: the two tensors the relocation rewrites
_MCMC_MAX_ROWS = 1 << 24                  # torch.multinomial takes at most 2^24 categories


class MCMCController(DensityController):
    """Training at a fixed budget of Gaussians, without opacity resets:

        ctrl = MCMCController(gaussians, optimizer, MCMCConfig(cap_max=...))
        ... per iteration:  (loss + ctrl.regularizer()).backward(); optimizer.step(); ctrl.step(it, xyz_lr)

    step() relocates the dead Gaussians onto live ones and grows the set by 5 % on the refinement schedule, and adds
    covariance-shaped noise to the positions on every call.  The optimizer is the one DensityController takes; its
    groups and state are kept as that class keeps them (_names, _state, _swap).  Only the methods below are served:
    the clone / split / delete step of the base class reads a DensifyConfig."""

    def __init__(self, gaussians, optimizer, config=None):
        super().__init__(gaussians, optimizer, config if config is not None else MCMCConfig())

    def _guard(self, what):
        """raises before anything is enqueued; -> the row count"""
        g = self.gaussians
        N = g.xyz.shape[0]
        if N > _MCMC_MAX_ROWS:
            raise RuntimeError(f"{what}: {N} Gaussians are more than 2^24, the limit of torch.multinomial")
        if self.config.cap_max < N:
            raise RuntimeError(f"{what}: cap_max {self.config.cap_max} is below the current count {N}")
        for k in self._names():
            t = getattr(g, k)
            if t.dtype != torch.float32 or not t.is_cuda:
                raise RuntimeError(f"{what} needs float32 tensors on the GPU: {k} is {t.dtype} on {t.device}")
            if not t.is_contiguous() or t.shape[0] != N:
                raise RuntimeError(f"{what} needs contiguous tensors of {N} rows: {k} is not")
        return N

    @staticmethod
    def _draw(sample, probs, n):
        rows = sample(probs, n) if sample is not None else torch.multinomial(probs, n, replacement=True)
        if rows.dtype != torch.int64 or tuple(rows.shape) != (n,) or rows.device != probs.device:
            raise RuntimeError(f"sample(probs, n) must return int64[{n}] on {probs.device}")
        return rows

    def opacity_floor(self):
        """the smallest opacity a relocated Gaussian gets (gs_mcmc_relocate's min_opacity): min_opacity raised by two
        fp32 steps of its logit, so that the stored logit lies above the dead threshold and a relocated row is alive by
        relocate's own `<=` (at min_opacity itself it would be dead again at once).  The c_float of the C ABI moves
        the logit by 0.13 of a step at most."""
        dead_logit = torch.tensor(inverse_sigmoid(self.config.min_opacity), dtype=torch.float32)
        step = torch.tensor(math.inf, dtype=torch.float32)
        above = torch.nextafter(torch.nextafter(dead_logit, step), step)
        return 1.0 / (1.0 + math.exp(-float(above)))

    def _relocate_call(self, names, params, exp_avg, exp_avg_sq, ratio, dst_rows, src_rows):
        n = len(names)
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])
        widths = (ctypes.c_int32 * n)(*[int(math.prod(t.shape[1:])) for t in params])
        kinds = (ctypes.c_int32 * n)(*[_MCMC_KIND.get(k, 0) for k in names])
        _hip.call("gs_mcmc_relocate", n, arr(params), arr(exp_avg), arr(exp_avg_sq), widths, kinds, params[0].shape[0],
                  _p(ratio), _p(dst_rows), _p(src_rows), dst_rows.shape[0], self.opacity_floor(),
                  _hip.current_stream())

    def _moments(self, name):
        st = self._state(name)
        if not (bool(st) and "exp_avg" in st):
            return None, None
        if not (st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous()):
            raise RuntimeError(f"MCMC densification needs contiguous optimizer moments: those of {name} are not")
        return st["exp_avg"], st["exp_avg_sq"]

    @staticmethod
    def _ratio(n_rows, src_rows):
        """1 + how often each row was drawn: torch.bincount(src_rows, minlength=n_rows) + 1 as int32, formed without
        bincount's host read"""
        ratio = torch.ones(n_rows, dtype=torch.int32, device=src_rows.device)
        return ratio.index_add_(0, src_rows, torch.ones_like(src_rows, dtype=torch.int32))

    @torch.no_grad()
    def relocate(self, sample=None):
        """Moves every dead Gaussian (opacity <= min_opacity, compared as logits) onto a live one drawn with probability
        proportional to its opacity, with replacement; a Gaussian drawn n - 1 times and its n - 1 copies get the
        opacity and scale that leave the image unchanged (gs_mcmc_relocate).  In place: parameter objects, optimizer
        keys and step counts stay; the moments of sources and destinations become 0 (other
        implementations keep the dead row's moments); the gradient accumulators are reset.  One host read (the dead
        count).  sample(probs, n) -> int64[n] with entries in [0, len(probs)), not checked, replaces
        torch.multinomial (tests).  -> {"relocated", "n_before", "n_after"}"""
        g, cfg = self.gaussians, self.config
        N = self._guard("relocate")
        info = self.last_info = dict(relocated=0, n_before=N, n_after=N)
        logit = g.opacity.detach().reshape(N)
        dead = logit <= inverse_sigmoid(cfg.min_opacity)
        n_dead = int(dead.sum().item())   # the host read
        if n_dead == 0 or n_dead == N:
            return info
        order = torch.argsort(dead.to(torch.uint8), descending=True, stable=True)   # dead rows first, each part in order
        dst_rows, alive_rows = order[:n_dead], order[n_dead:]
        src_rows = alive_rows[self._draw(sample, torch.sigmoid(logit[alive_rows]), n_dead)]
        names = self._names()
        moments = [self._moments(k) for k in names]
        self._relocate_call(names, [getattr(g, k).detach() for k in names], [m for m, _ in moments],
                            [v for _, v in moments], self._ratio(N, src_rows), dst_rows.to(torch.int32),
                            src_rows.to(torch.int32))
        self.reset_grad_accum()
        info["relocated"] = n_dead
        return info

    @torch.no_grad()
    def add_new(self, sample=None):
        """Grows the set to min(cap_max, int(grow_factor * N)) rows: the new rows are copies of Gaussians drawn as in
        relocate (from all rows), corrected the same way.  One gs_densify_move with the identity as destination fills
        the first N rows of the new tensors and moments, one gs_mcmc_relocate the appended ones; the optimizer groups
        are re-keyed, the step counts kept, the gradient accumulators reset.  No host read.  -> {"added", "n_before",
        "n_after"}"""
        g, cfg = self.gaussians, self.config
        N = self._guard("add_new")
        n_add = max(0, min(cfg.cap_max, int(cfg.grow_factor * N)) - N)
        info = self.last_info = dict(added=n_add, n_before=N, n_after=N + n_add)
        if n_add == 0:
            return info
        dev = g.xyz.device
        src_rows = self._draw(sample, torch.sigmoid(g.opacity.detach().reshape(N)), n_add)
        names = self._names()
        src, dst, src_m, dst_m, src_v, dst_v = [], [], [], [], [], []
        for k in names:
            t = getattr(g, k).detach()
            m, v = self._moments(k)
            src.append(t)
            dst.append(torch.empty((N + n_add,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev))
            src_m.append(m)
            src_v.append(v)
            dst_m.append(torch.empty_like(dst[-1]) if m is not None else None)
            dst_v.append(torch.empty_like(dst[-1]) if m is not None else None)
        n = len(names)
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])
        widths = (ctypes.c_int32 * n)(*[int(math.prod(t.shape[1:])) for t in src])
        kinds = (ctypes.c_int32 * n)(*[_KIND.get(k, 0) for k in names])
        xyz_s, scale_s, quat_s = (src[names.index(k)] for k in ("xyz", "scale", "quaternion"))
        identity = torch.arange(N, dtype=torch.int32, device=dev)
        minus = torch.full((N,), -1, dtype=torch.int32, device=dev)
        no_samples = torch.zeros(1, 3, device=dev)   # (n_split == 0: never read)
        _hip.call("gs_densify_move", n, arr(src), arr(dst), arr(src_m), arr(dst_m), arr(src_v), arr(dst_v), widths,
                  kinds, N, _p(identity), _p(minus), _p(minus), _p(minus), _p(xyz_s), _p(scale_s), _p(quat_s),
                  _p(self.xyz_grad_accum), _p(self.grad_accum_count), _p(no_samples), 0, 0, N, 1.0,
                  _hip.current_stream())
        new_rows = torch.arange(N, N + n_add, dtype=torch.int32, device=dev)
        self._relocate_call(names, dst, dst_m, dst_v, self._ratio(N + n_add, src_rows), new_rows,
                            src_rows.to(torch.int32))
        for k, d, m, v in zip(names, dst, dst_m, dst_v):
            self._swap(k, d, m, v)
        self.reset_grad_accum()
        return info

    @torch.no_grad()
    def inject_noise(self, xyz_lr, noise=None):
        """xyz += Sigma_world (noise * gate(opacity) * noise_lr * xyz_lr) in place, one launch (gs_mcmc_add_noise).
        noise: [N, 3] standard normal samples (default: torch.randn_like(xyz))"""
        g, cfg = self.gaussians, self.config
        N = self._guard("inject_noise")
        xyz = g.xyz.detach()
        if noise is None:
            noise = torch.randn_like(xyz)
        elif not (torch.is_tensor(noise) and noise.dtype == torch.float32 and tuple(noise.shape) == (N, 3)
                  and noise.device == xyz.device and noise.is_contiguous()):
            raise RuntimeError(f"inject_noise: noise must be a contiguous float32 [{N}, 3] tensor on {xyz.device}")
        _hip.call("gs_mcmc_add_noise", _p(xyz), _p(g.quaternion.detach()), _p(g.scale.detach()), _p(g.opacity.detach()),
                  _p(noise), N, cfg.noise_lr * xyz_lr, cfg.gate_k, cfg.gate_x0, _hip.current_stream())

    def regularizer(self):
        """opacity_reg * mean(sigmoid(opacity)) + scale_reg * mean(exp(scale)): differentiable, to be added to the loss
        (it is what makes Gaussians die, so that relocate has something to move)"""
        g, cfg = self.gaussians, self.config
        return cfg.opacity_reg * torch.sigmoid(g.opacity).mean() + cfg.scale_reg * torch.exp(g.scale).mean()

    @torch.no_grad()
    def step(self, it, xyz_lr):
        """The schedule, after optimizer.step() of iteration `it`: relocate() then add_new() when refine_start < it <
        refine_stop and it % refine_every == 0, inject_noise(xyz_lr) on every call.  -> {"refined", "relocated",
        "added", "n_before", "n_after"}"""
        cfg = self.config
        N = self.gaussians.xyz.shape[0]
        info = dict(refined=False, relocated=0, added=0, n_before=N, n_after=N)
        if cfg.refine_start < it < cfg.refine_stop and it % cfg.refine_every == 0:
            moved, grown = self.relocate(), self.add_new()
            info.update(refined=True, relocated=moved["relocated"], added=grown["added"], n_after=grown["n_after"])
        self.inject_noise(xyz_lr)
        self.last_info = info
        return info
