"""MCMC densification on the device (csrc/mcmc.hip, densify.MCMCController) against the float64 references and the
plain-torch restatement of tests/mcmc_ref.py.

Relocation: every rewritten opacity and scale within ONE fp32 ulp of the float64 reference rounded to fp32 -- both sides
are double evaluations accurate to ~1e-11 (tests/test_mcmc_ref.py), four orders below half an fp32 ulp, so they differ
only where the exact value lies on a rounding boundary; everything the kernel does not rewrite, bit for bit.
Noise: in units of eps32 * M (M: the summed magnitudes of the three products of an element), at most 4x what the fp32
CPU restatement of the same arithmetic shows on the same inputs (device division and the fmaf of the exponential differ
from the host's in last bits, and the gate amplifies an error of its argument a hundredfold)."""
import ctypes
import math

import pytest
import torch

from gaussian_splatting_amd import _hip, fused
from gaussian_splatting_amd.densify import MCMCConfig, MCMCController, inverse_sigmoid
from gaussian_splatting_amd.splat_py.structs import Gaussians
from gaussian_splatting_amd.synthetic import DEFAULTS, make_scene
from gaussian_splatting_amd.train_ops import Adam, ssim_l1_loss

from . import mcmc_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
LRS = dict(xyz=2e-4, quaternion=4e-3, scale=1e-2, opacity=2e-2, rgb=4e-3, sh=2e-4)
MIN_OPACITY = 0.005


def bits(t):
    return t.contiguous().view(torch.int32)


def ulps(a, b):
    """distance of two fp32 tensors in units of the last place (monotone integer image of the floats)"""
    def key(t):
        i = bits(t).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return (key(a) - key(b)).abs()


def relocate_raw(params, exp_avg, exp_avg_sq, kinds, ratio, dst_rows, src_rows, min_opacity=MIN_OPACITY):
    """gs_mcmc_relocate on lists of tensors (None: no moments) -> the status"""
    n = len(params)
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])
    widths = (ctypes.c_int32 * n)(*[int(math.prod(t.shape[1:])) for t in params])
    kind = (ctypes.c_int32 * n)(*kinds)
    m = 0 if dst_rows is None else dst_rows.shape[0]
    status = _hip.lib().gs_mcmc_relocate(n, arr(params), arr(exp_avg), arr(exp_avg_sq), widths, kind, params[0].shape[0],
                                         _hip.ptr(ratio), _hip.ptr(dst_rows), _hip.ptr(src_rows), m, min_opacity,
                                         _hip.current_stream())
    torch.cuda.synchronize()
    return status


def test_relocation_values_within_one_ulp_and_untouched_rows_keep_every_bit():
    n_rows = 1000   # not a multiple of 256
    gen = torch.Generator().manual_seed(3)
    ratios = (1, 2, 3, 50, 51, 52, 1000)
    special = (-20.0, 20.0, 0.0, inverse_sigmoid(MIN_OPACITY))
    logit = 3.0 * torch.randn(n_rows, 1, generator=gen)
    ratio = torch.tensor([ratios[r % 7] for r in range(n_rows)], dtype=torch.int32)
    for j, x in enumerate(special):          # every special logit with every ratio
        logit[7 * j: 7 * j + 7, 0] = x
    ratio[n_rows - 1] = 1                    # the one destination (the call launches only with M > 0)
    scale = torch.rand(n_rows, 3, generator=gen) * 7.0 - 6.0
    untouched = torch.nonzero(ratio == 1).flatten()[:-1]
    logit[untouched[0], 0] = math.nan        # rows the kernel must not read, let alone write
    scale[untouched[1], 2] = math.inf
    moments = [torch.randn(n_rows, w, generator=gen) for w in (1, 1, 3, 3)]
    moments[0][untouched[2], 0] = math.nan
    moments[3][untouched[3], 1] = -math.inf
    logit, scale, ratio = logit.to(DEV), scale.to(DEV), ratio.to(DEV)
    m_o, v_o, m_s, v_s = (t.to(DEV) for t in moments)
    before = [t.clone() for t in (logit, scale, m_o, v_o, m_s, v_s)]
    src_row = 8   # ratio 2
    assert int(ratio[src_row]) == 2
    dst = torch.tensor([n_rows - 1], dtype=torch.int32, device=DEV)
    src = torch.tensor([src_row], dtype=torch.int32, device=DEV)
    assert relocate_raw([logit, scale], [m_o, m_s], [v_o, v_s], [4, 2], ratio, dst, src) == _hip.GS_OK

    hit = torch.nonzero(ratio > 1).flatten()
    new_logit, shift, _, _ = M.relocation(before[0][hit, 0], ratio[hit], MIN_OPACITY)
    want_logit = new_logit.float()
    want_scale = (before[1][hit].double() + shift[:, None]).float()
    d_o, d_s = ulps(logit[hit, 0], want_logit), ulps(scale[hit], want_scale)
    print("relocation: %d rows rewritten, opacity off by one ulp in %d, scale elements in %d of %d"
          % (hit.numel(), int((d_o > 0).sum()), int((d_s > 0).sum()), d_s.numel()))
    assert bool(torch.isfinite(logit[hit]).all()) and bool(torch.isfinite(scale[hit]).all())
    assert int(d_o.max()) <= 1 and int(d_s.max()) <= 1, (int(d_o.max()), int(d_s.max()))
    assert bool((scale[hit] <= before[1][hit]).all())   # no copy grows
    for t in (m_o, v_o, m_s, v_s):
        assert bool((t[hit] == 0).all())
    for t, t0 in zip((logit, scale, m_o, v_o, m_s, v_s), before):   # ratio 1: every bit, NaN payloads included
        assert torch.equal(bits(t[untouched]), bits(t0[untouched]))
    # the destination holds the corrected source, its moments are 0
    assert torch.equal(bits(logit[-1]), bits(logit[src_row])) and torch.equal(bits(scale[-1]), bits(scale[src_row]))
    assert all(bool((t[-1] == 0).all()) for t in (m_o, v_o, m_s, v_s))


def move_case():
    n_rows = 777
    gen = torch.Generator().manual_seed(9)
    widths, kinds = (3, 4, 3, 1, 3, 45), (0, 0, 2, 4, 0, 0)
    params = [torch.randn(n_rows, w, generator=gen).to(DEV) for w in widths]
    has = (True, True, True, True, False, True)   # the fifth tensor has no moments
    ms = [torch.randn(n_rows, w, generator=gen).to(DEV) if h else None for w, h in zip(widths, has)]
    vs = [torch.rand(n_rows, w, generator=gen).to(DEV) if h else None for w, h in zip(widths, has)]
    perm = torch.randperm(n_rows, generator=gen)
    sources = perm[:20]
    src = sources.repeat(3)[torch.randperm(60, generator=gen)]   # every source three times, in no order
    dst = perm[20:80]
    ratio = (torch.bincount(src, minlength=n_rows) + 1).to(torch.int32)
    return params, ms, vs, kinds, ratio.to(DEV), dst.to(torch.int32).to(DEV), src.to(torch.int32).to(DEV)


def test_move_copies_rows_zeroes_moments_and_leaves_the_rest():
    params, ms, vs, kinds, ratio, dst, src = move_case()
    before = [[None if t is None else t.clone() for t in ts] for ts in (params, ms, vs)]
    assert relocate_raw(params, ms, vs, kinds, ratio, dst, src) == _hip.GS_OK
    dl, sl = dst.long(), src.long()
    rest = torch.ones(params[0].shape[0], dtype=torch.bool, device=DEV)
    rest[dl] = False
    rest[sl] = False
    for k, p in enumerate(params):
        assert torch.equal(bits(p[dl]), bits(p[sl])), k            # destination == source as the call left it
        assert torch.equal(bits(p[rest]), bits(before[0][k][rest])), k
        if kinds[k] == 0:
            assert torch.equal(bits(p[sl]), bits(before[0][k][sl])), k   # plain tensors: the sources themselves stay
        else:
            assert not torch.equal(p[sl], before[0][k][sl]), k
        if ms[k] is None:
            continue
        for t, t0 in ((ms[k], before[1][k]), (vs[k], before[2][k])):
            assert bool((t[dl] == 0).all()) and bool((t[sl] == 0).all()), k
            assert torch.equal(bits(t[rest]), bits(t0[rest])), k


def test_empty_call_and_missing_scale_tensor():
    params, ms, vs, kinds, ratio, dst, src = move_case()
    before = [t.clone() for t in params]
    assert relocate_raw(params, ms, vs, kinds, ratio, None, None) == _hip.GS_OK   # M == 0: nothing is launched
    assert relocate_raw(params, ms, vs, kinds, ratio, dst[:0], src[:0]) == _hip.GS_OK
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(params, before))
    no_scale = [0, 0, 0, 4, 0, 0]
    assert relocate_raw(params, ms, vs, no_scale, ratio, dst, src) == _hip.GS_EINVAL
    assert b"one scale tensor" in _hip.lib().gs_last_error()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(params, before))


# ---- noise ------------------------------------------------------------------------------------------------------------
STEP, GATE_K, GATE_X0 = 5e5 * 1.6e-4, 100.0, 0.995
# an element whose products lie this far above fp32's smallest normal number: no underflow inside an fp32 evaluation
NORMAL_RANGE = 2.0 ** -100


def noise_inputs(N):
    gen = torch.Generator().manual_seed(100 + N)
    q = torch.randn(N, 4, generator=gen)                                    # not normalised
    s = torch.rand(N, 3, generator=gen) * 7.0 - 6.0                         # [-6, 1]
    o = torch.exp(torch.linspace(math.log(1e-4), math.log(0.999), N, dtype=torch.float64))
    logit = torch.log(o / (1.0 - o)).float().reshape(N, 1)[torch.randperm(N, generator=gen)]
    noise = torch.randn(N, 3, generator=gen)
    xyz = 10.0 * torch.randn(N, 3, generator=gen)
    return [t.contiguous() for t in (q, s, logit, noise, xyz)]


def add_noise(xyz, q, s, logit, noise):
    p = _hip.ptr
    _hip.call("gs_mcmc_add_noise", p(xyz), p(q), p(s), p(logit), p(noise), xyz.shape[0], STEP, GATE_K, GATE_X0,
              _hip.current_stream())
    torch.cuda.synchronize()
    return xyz


@pytest.mark.parametrize("N", [0, 257, 1000])
def test_noise_against_float64_and_bit_exact_accumulation(N):
    """Measured on the MI355X, in units of eps32 * M: on the elements whose products are in fp32's normal range the fp32
    CPU restatement lies 77.47 (N = 257) and 87.46 (N = 1000) from the float64 reference, and the kernel the same 77.47
    and 87.46: its exponential is IEEE-only, so it reproduces the restatement; allowed are 4x the restatement's figure.
    On all elements both show 8.389e6 = 2^23: an opacity above ~0.88 makes expf overflow in fp32, the gate is exactly 0
    there while float64 still gives ~1e-39, and the unit itself underflows.  The comparison over all elements is what
    the feature's issue set and stays; the one over the normal range is the one that binds.  See DESIGN.md 7h."""
    q, s, logit, noise, xyz0 = noise_inputs(N)
    dq, ds, dl, dn = (t.to(DEV) for t in (q, s, logit, noise))
    d = add_noise(torch.zeros(N, 3, device=DEV), dq, ds, dl, dn)
    if N == 0:
        assert d.shape == (0, 3)
        return
    assert bool(torch.isfinite(d).all())
    ref, mag = M.noise_displacement(q, s, logit, noise, STEP, GATE_K, GATE_X0)
    cpu32 = M.noise_fp32(q, s, logit, noise, STEP, GATE_K, GATE_X0)
    normal = mag > NORMAL_RANGE
    assert int(normal.sum()) > 0.8 * mag.numel() and float(ref.abs().max()) > 1.0
    for name, rows in (("all elements", torch.ones_like(normal)), ("normal range", normal)):
        yardstick = M.error_multiple(cpu32[rows], ref[rows], mag[rows])
        got = M.error_multiple(d.cpu()[rows], ref[rows], mag[rows])
        print("noise N=%d, %s: kernel %.4g, fp32 CPU restatement %.4g (units of eps32 * M)" % (N, name, got, yardstick))
        assert got <= 4.0 * yardstick, (name, got, yardstick)
    # one IEEE add per element: xyz + d, bit for bit
    out = add_noise(xyz0.to(DEV), dq, ds, dl, dn)
    assert torch.equal(bits(out), bits(xyz0.to(DEV) + d))


# ---- the controller ---------------------------------------------------------------------------------------------------
def build(N, seed, cap_max, deg=1, n_dead=0):
    g, cam, T = make_scene(N, 96, 96, deg, seed=seed, device=DEV)
    gen = torch.Generator().manual_seed(seed + 1)
    if n_dead:   # make_scene's logits are N(0, 2): hardly any is below -5.3 on its own
        g.opacity[torch.randperm(N, generator=gen)[:n_dead].to(DEV)] = -7.0
    params = [getattr(g, k) for k in NAMES if getattr(g, k) is not None]
    for p in params:
        p.requires_grad_(True)
    opt = Adam([{"params": getattr(g, k), "lr": LRS[k]} for k in NAMES if getattr(g, k) is not None])
    dgen = torch.Generator(device=DEV).manual_seed(seed + 2)
    for _ in range(3):   # non-trivial moments
        for p in params:
            p.grad = torch.randn(p.shape, generator=dgen, device=DEV) * 1e-3
        opt.step()
    opt.zero_grad(set_to_none=True)
    return g, opt, MCMCController(g, opt, MCMCConfig(cap_max=cap_max, min_opacity=MIN_OPACITY)), cam, T


def snapshot(g, opt):
    names = [k for k in NAMES if getattr(g, k) is not None]
    p = {k: getattr(g, k).detach().clone() for k in names}
    m = {k: opt.state[getattr(g, k)]["exp_avg"].clone() for k in names}
    v = {k: opt.state[getattr(g, k)]["exp_avg_sq"].clone() for k in names}
    return p, m, v


def compare_with_restatement(g, opt, p, m, v, ratio):
    """parameters: opacity and scale of the rows the relocation wrote within one ulp of the restatement, everything else
    bit for bit; moments bit for bit"""
    for k in p:
        got = getattr(g, k).detach()
        assert got.shape == p[k].shape, k
        if k in ("opacity", "scale"):
            assert int(ulps(got, p[k]).max()) <= 1, k
        else:
            assert torch.equal(bits(got), bits(p[k])), k
        st = opt.state[getattr(g, k)]
        assert torch.equal(bits(st["exp_avg"]), bits(m[k])) and torch.equal(bits(st["exp_avg_sq"]), bits(v[k])), k
    for i, k in enumerate(k for k in NAMES if getattr(g, k) is not None):
        assert opt.param_groups[i]["params"][0] is getattr(g, k)


def step_once(g, opt, seed):
    dgen = torch.Generator(device=DEV).manual_seed(seed)
    for k in NAMES:
        p = getattr(g, k)
        if p is not None:
            p.grad = torch.randn(p.shape, generator=dgen, device=DEV) * 1e-3
    opt.step()
    opt.zero_grad(set_to_none=True)
    assert all(bool(torch.isfinite(getattr(g, k)).all()) for k in NAMES if getattr(g, k) is not None)


def test_controller_relocate_matches_the_restatement():
    N, n_dead = 2000, 150
    g, opt, ctrl, cam, T = build(N, seed=21, cap_max=5000, n_dead=n_dead)
    objects = {k: getattr(g, k) for k in NAMES}
    steps = {k: float(opt.state[getattr(g, k)]["step"]) for k in NAMES}
    p, m, v = snapshot(g, opt)
    thr = inverse_sigmoid(MIN_OPACITY)
    dead_before = int((g.opacity.detach() <= thr).sum())
    assert dead_before >= n_dead
    drawn = {}

    def sample(probs, n):   # few sources, so that many are drawn several times
        assert probs.shape == (N - dead_before,) and n == dead_before and bool((probs > 0).all())
        drawn["rows"] = torch.randint(0, 40, (n,), generator=torch.Generator().manual_seed(4)).to(DEV)
        return drawn["rows"]

    ctrl.uv_grad_accum += 1.0
    info = ctrl.relocate(sample)
    assert info == dict(relocated=dead_before, n_before=N, n_after=N)
    dst, src, ratio = M.relocate(p, m, v, drawn["rows"], MIN_OPACITY, ctrl.opacity_floor())
    assert int(ratio.max()) > 3
    assert all(getattr(g, k) is objects[k] for k in NAMES) and g.xyz.shape[0] == N
    compare_with_restatement(g, opt, p, m, v, ratio)
    for k in NAMES:   # a relocated row is its source, bit for bit; the step counts are kept
        t = getattr(g, k).detach()
        assert torch.equal(bits(t[dst]), bits(t[src])), k
        assert float(opt.state[getattr(g, k)]["step"]) == steps[k]
    assert int((g.opacity.detach() <= thr).sum()) == 0
    assert float(ctrl.uv_grad_accum.abs().sum()) == 0.0 and ctrl.uv_grad_accum.shape == (N, 2)
    # nothing dead: nothing to do, nothing sampled
    assert ctrl.relocate(lambda probs, n: pytest.fail("sampled without a dead row"))["relocated"] == 0
    step_once(g, opt, 5)


def test_controller_add_new_grows_to_the_cap_and_stops():
    N = 2000
    g, opt, ctrl, cam, T = build(N, seed=22, cap_max=2150)
    p, m, v = snapshot(g, opt)
    drawn = {}

    def sample(probs, n):
        assert probs.shape == (N,) and n == 100
        drawn["rows"] = torch.randint(0, 30, (n,), generator=torch.Generator().manual_seed(6)).to(DEV)
        return drawn["rows"]

    info = ctrl.add_new(sample)
    assert info == dict(added=int(1.05 * N) - N, n_before=N, n_after=2100)
    p, m, v = M.add_new(p, m, v, drawn["rows"], ctrl.opacity_floor())
    compare_with_restatement(g, opt, p, m, v, None)
    for k in NAMES:
        t = getattr(g, k).detach()
        assert torch.equal(bits(t[N:]), bits(t[drawn["rows"]])), k
    assert ctrl.grad_accum_count.shape == (2100,)
    step_once(g, opt, 7)
    assert ctrl.add_new() == dict(added=50, n_before=2100, n_after=2150)      # int(1.05 * 2100) = 2205: the cap decides
    assert g.xyz.shape[0] == 2150 == ctrl.config.cap_max
    assert ctrl.add_new(lambda probs, n: pytest.fail("sampled at the cap")) == dict(added=0, n_before=2150, n_after=2150)
    step_once(g, opt, 8)
    ctrl.config.cap_max = 2149
    with pytest.raises(RuntimeError, match="cap_max 2149 is below the current count 2150"):
        ctrl.add_new()


def test_controller_step_follows_the_schedule():
    g, opt, ctrl, cam, T = build(1000, seed=23, cap_max=1200, n_dead=30)
    ctrl.config.refine_start, ctrl.config.refine_every, ctrl.config.refine_stop = 2, 3, 8
    thr = inverse_sigmoid(MIN_OPACITY)
    dead = int((g.opacity.detach() <= thr).sum())
    assert dead >= 30
    for it in range(1, 11):
        before = {k: getattr(g, k).detach().clone() for k in NAMES}
        info = ctrl.step(it, 1.6e-4)
        refined = it in (3, 6)
        assert info["refined"] == refined, it
        if refined:
            assert info["n_after"] == min(1200, int(1.05 * info["n_before"])) == g.xyz.shape[0]
            assert info["relocated"] == (dead if it == 3 else 0) and int((g.opacity.detach() <= thr).sum()) == 0
        else:
            assert info["relocated"] == 0 and info["added"] == 0
            for k in NAMES:
                if k != "xyz":
                    assert torch.equal(bits(getattr(g, k).detach()), bits(before[k])), (it, k)
        n0 = before["xyz"].shape[0]
        assert not torch.equal(g.xyz.detach()[:n0], before["xyz"]), it     # noise on every call
    assert g.xyz.shape[0] == 1102
    step_once(g, opt, 9)


# ---- a short run --------------------------------------------------------------------------------------------------------
def test_short_training_run_at_a_fixed_budget():
    """400 iterations of fused.rasterize, SSIM + L1 + regularizer, Adam and MCMCController.step on a hidden scene of
    2 000 Gaussians at 96x96 from 8 poses, started from 500 of its centres (perturbed) with a budget of 1 500.
    Measured on the MI355X: training PSNR 17.23 -> 27.01 dB (gain 9.78 dB; a second run ended at 26.72) with 36
    refinements, 48 rows relocated and the budget reached at the 23rd; half of the gain is asserted, since the gradients
    are summed by atomics and runs differ."""
    import bench
    W = H = 96
    n_truth, n_start, cap, iters = 2000, 500, 1500, 400
    poses = bench.camera_poses(8, 4321, DEV, moving=True)
    truth, cam, _ = make_scene(n_truth, W, H, 0, seed=77, device=DEV)
    truth.scale += math.log(2.0)
    bg = torch.zeros(3, device=DEV)
    render = lambda gs, T: fused.rasterize(gs, T, cam, use_sh_precompute=True, background_rgb=bg, **DEFAULTS)[0]
    with torch.no_grad():
        targets = [render(truth, T).clamp(0, 1) for T in poses]
    gen = torch.Generator().manual_seed(5)
    pick = torch.randperm(n_truth, generator=gen)[:n_start].to(DEV)
    xyz = truth.xyz[pick] * (1.0 + 2e-3 * torch.randn(n_start, 3, generator=gen).to(DEV))
    rgb = truth.rgb[pick] + 0.1 * torch.randn(n_start, 3, generator=gen).to(DEV)
    quat = torch.zeros(n_start, 4, device=DEV)
    quat[:, 0] = 1.0
    g = Gaussians(xyz.contiguous(), rgb.contiguous(), torch.full((n_start, 1), inverse_sigmoid(0.5), device=DEV),
                  truth.scale[pick].mean(dim=1, keepdim=True).expand(n_start, 3).contiguous(), quat, None)
    names = ("xyz", "quaternion", "scale", "opacity", "rgb")
    for k in names:
        getattr(g, k).requires_grad_(True)
    opt = Adam([{"params": getattr(g, k), "lr": LRS[k]} for k in names])
    ctrl = MCMCController(g, opt, MCMCConfig(cap_max=cap, refine_start=20, refine_every=10, refine_stop=iters - 10))
    thr = inverse_sigmoid(ctrl.config.min_opacity)

    def psnr():
        with torch.no_grad():
            mse = torch.stack([ssim_l1_loss(render(g, T).clamp(0, 1), tgt, 0.2, return_terms=True)[1][3]
                               for T, tgt in zip(poses, targets)])
            return float((-10.0 * torch.log10(mse.double())).mean())

    start = psnr()
    order = torch.randint(0, 8, (iters,), generator=gen).tolist()
    counts, refinements, relocated, dead_after_last = [], 0, 0, None
    for it in range(1, iters + 1):
        opt.zero_grad(set_to_none=True)
        c = order[it - 1]
        (ssim_l1_loss(render(g, poses[c]), targets[c], 0.2) + ctrl.regularizer()).backward()
        opt.step()
        info = ctrl.step(it, LRS["xyz"])
        if info["refined"]:
            refinements += 1
            relocated += info["relocated"]
            dead_after_last = (g.opacity.detach() <= thr).sum()   # (read after the loop)
            counts.append(info["n_after"])
    end = psnr()
    print("short run: PSNR %.3f -> %.3f dB, %d refinements, %d relocated, counts %s"
          % (start, end, refinements, relocated, counts[:3] + counts[-3:]))
    assert refinements == 36 and counts[0] == 525
    assert max(counts) <= cap and g.xyz.shape[0] == cap
    assert int(dead_after_last) == 0
    assert all(bool(torch.isfinite(getattr(g, k)).all()) for k in names)
    for k in names:
        st = opt.state[getattr(g, k)]
        assert bool(torch.isfinite(st["exp_avg"]).all()) and bool(torch.isfinite(st["exp_avg_sq"]).all())
        assert st["exp_avg"].shape == getattr(g, k).shape
    assert end > start
    assert end - start > 0.5 * MEASURED_GAIN_DB, (start, end)


MEASURED_GAIN_DB = 9.78   # the short run's measured gain (its docstring)
