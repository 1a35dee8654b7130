"""References for MCMC densification (csrc/mcmc.hip, densify.MCMCController), plain torch on the CPU or wherever the
inputs live:

  relocation            opacity and scale of a Gaussian that stands for one of n copies, float64, with the published
                        double sum (3DGS-MCMC eq. 9) -- the kernel evaluates its hockey-stick form
  noise_displacement    Sigma_world (noise * gate * step) in float64, with the magnitudes of the three products per element
  noise_fp32            the same arithmetic in fp32 in the kernel's operation order (det_expf restated): the yardstick of
                        how far an fp32 evaluation lies from the float64 one
  relocate / add_new    the controller's two refinement steps on dicts of parameters and moments
"""
import math

import torch

MAX_RATIO = 51
O_MAX = 1.0 - 2.0 ** -24
F32_EPS = 2.0 ** -23


# ---- relocation ---------------------------------------------------------------------------------------------------
def denom_double_sum(o_new, n):
    """sum_{i=1..n} sum_{k=0..i-1} C(i-1,k) (-1)^k o_new^(k+1) / sqrt(k+1), as published; o_new: float64 tensor"""
    total = torch.zeros_like(o_new)
    for i in range(1, n + 1):
        for k in range(i):
            total = total + float(math.comb(i - 1, k)) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1)
    return total


def denom_hockey_stick(o_new, n):
    """sum_{k=0..n-1} C(n,k+1) (-1)^k o_new^(k+1) / sqrt(k+1): the same value (sum_{i>k} C(i-1,k) = C(n,k+1))"""
    total = torch.zeros_like(o_new)
    for k in range(n):
        total = total + float(math.comb(n, k + 1)) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1)
    return total


def opacity_new(o, n):
    """1 - (1 - o)^(1/n) as -expm1(log1p(-o) / n): the same function, without the cancellation at small o"""
    return -torch.expm1(torch.log1p(-o) / n)


def relocation(logit, ratio, min_opacity, denom_of=denom_double_sum):
    """logit: fp32 [R], ratio: int [R] (every entry > 1) -> float64 (new logit [R], log-scale offset [R], o_new, denom)"""
    x = logit.double()
    o = torch.clamp(1.0 / (1.0 + torch.exp(-x)), max=O_MAX)
    n_all = torch.clamp(ratio.to(torch.int64), max=MAX_RATIO)
    o_new, denom = torch.zeros_like(o), torch.ones_like(o)
    for n in sorted(set(n_all.tolist())):
        rows = n_all == n
        o_new[rows] = opacity_new(o[rows], n)
        denom[rows] = denom_of(o_new[rows], n)
    oc = torch.clamp(o_new, min=float(torch.tensor(min_opacity, dtype=torch.float32)), max=O_MAX)   # as the C ABI gets it
    return torch.log(oc / (1.0 - oc)), torch.log(o / denom), o_new, denom


# ---- noise ----------------------------------------------------------------------------------------------------------
def _rotation(w, x, y, z):   # pg_math.h quat_to_rot, its operation order
    return [1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
            2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
            2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]


def _sigma_world(q, s, exp):   # pg_math.h sigma_world_of, its operation order (in the dtype of q and s)
    w, x, y, z = q.unbind(1)
    norm = torch.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / norm, y / norm, z / norm, w / norm
    r = _rotation(w, x, y, z)
    sx, sy, sz = (exp(c) for c in s.unbind(1))
    s2 = (sx * sx, sy * sy, sz * sz)
    S = {}
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        S[a, b] = S[b, a] = (r[3 * a] * r[3 * b] * s2[0] + r[3 * a + 1] * r[3 * b + 1] * s2[1]) \
            + r[3 * a + 2] * r[3 * b + 2] * s2[2]
    return S


def _displacement(q, s, logit, noise, step, gate_k, gate_x0, exp):
    one = torch.ones((), dtype=q.dtype)
    o = one / (one + exp(-logit.reshape(-1)))
    gate = one / (one + exp(-gate_k * ((one - o) - gate_x0)))
    S = _sigma_world(q, s, exp)
    f = gate * step
    e = [noise[:, c] * f for c in range(3)]
    d, mag = [], []
    for r in range(3):
        t = [S[r, c] * e[c] for c in range(3)]
        d.append((t[0] + t[1]) + t[2])
        mag.append(t[0].abs() + t[1].abs() + t[2].abs())
    return torch.stack(d, dim=1), torch.stack(mag, dim=1)


def noise_displacement(q, s, logit, noise, step, gate_k, gate_x0):
    """float64 reference of gs_mcmc_add_noise's displacement: the fp32 inputs (step, gate_k, gate_x0 as the fp32 values
    the C ABI receives) evaluated in float64 -> (d [N,3], M [N,3] = the summed magnitudes of the three products of d)"""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    return _displacement(q.double(), s.double(), logit.double(), noise.double(), f32(step), f32(gate_k), f32(gate_x0),
                         torch.exp)


def det_expf(x):
    """gs_common.h det_expf on an fp32 CPU tensor, operation by operation; each fmaf is formed as the fp32 rounding of
    the float64 sum of the exact product (a double rounding: it can differ from the fused result in rare last bits)"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()
    t = x * f32(1.44269504088896341)
    tc = torch.clamp(t, -126.0, 127.0)
    n = torch.round(tc)   # half to even, as rintf
    f = tc - n
    p = f32(1.54035303933816e-4).expand_as(f)
    for c in (1.33335581464284e-3, 9.61812910762848e-3, 5.55041086648216e-2, 2.40226506959101e-1, 6.93147180559945e-1,
              1.0):
        p = fma(p, f, f32(c))
    r = torch.ldexp(p, n.to(torch.int32))
    r = torch.where(t > 127.0, torch.full_like(r, math.inf), r)
    r = torch.where(t > -125.0, r, torch.zeros_like(r))
    return torch.where(t != t, t, r)


def noise_fp32(q, s, logit, noise, step, gate_k, gate_x0):
    """the displacement in fp32 in the kernel's operation order, on the CPU -> d [N,3] fp32"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    cpu = lambda t: t.detach().float().cpu()
    return _displacement(cpu(q), cpu(s), cpu(logit), cpu(noise), f32(step), f32(gate_k), f32(gate_x0), det_expf)[0]


def error_multiple(d, ref, mag):
    """the largest |d - ref| in units of eps32 * M (elements whose three products are all 0 count as 0)"""
    err = (d.double().cpu() - ref.cpu()).abs() / (F32_EPS * mag.cpu()).clamp(min=1e-300)
    return float(err[mag.cpu() > 0].max()) if bool((mag > 0).any()) else 0.0


# ---- the controller's steps on plain tensors ------------------------------------------------------------------------
def _apply_relocation(p, m, v, ratio, dst_rows, src_rows, min_opacity):
    """in place on the dicts' tensors: the sampled rows corrected, their moments zeroed, then copied over dst_rows"""
    hit = torch.nonzero(ratio > 1).flatten()
    if hit.numel():
        new_logit, log_ratio, _, _ = relocation(p["opacity"][hit, 0], ratio[hit], min_opacity)
        p["opacity"][hit, 0] = new_logit.float()
        p["scale"][hit] = (p["scale"][hit].double() + log_ratio[:, None]).float()
    for k in p:
        if k in m:
            m[k][hit] = 0.0
            v[k][hit] = 0.0
        p[k][dst_rows] = p[k][src_rows]
        if k in m:
            m[k][dst_rows] = 0.0
            v[k][dst_rows] = 0.0


def relocate(p, m, v, src_of_dead, min_opacity, floor):
    """MCMCController.relocate with the draw given: src_of_dead[j] = index AMONG THE ALIVE ROWS of the source of the
    j-th dead row; floor: the controller's opacity_floor().  p, m, v: dicts name -> tensor (m, v only for the tensors
    that have moments), modified in place.  -> (dst_rows, src_rows, ratio)"""
    n = p["opacity"].shape[0]
    dead = p["opacity"][:, 0] <= math.log(min_opacity / (1.0 - min_opacity))
    dst_rows, alive = torch.nonzero(dead).flatten(), torch.nonzero(~dead).flatten()
    src_rows = alive[src_of_dead]
    ratio = torch.bincount(src_rows, minlength=n) + 1
    _apply_relocation(p, m, v, ratio, dst_rows, src_rows, floor)
    return dst_rows, src_rows, ratio


def add_new(p, m, v, src_rows, floor):
    """MCMCController.add_new with the draw given: -> new dicts (p, m, v) of N + len(src_rows) rows"""
    n, n_add = p["opacity"].shape[0], src_rows.shape[0]
    grow = lambda t: torch.cat([t, torch.zeros((n_add,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)], dim=0)
    p, m, v = ({k: grow(t) for k, t in d.items()} for d in (p, m, v))
    ratio = torch.bincount(src_rows, minlength=n + n_add) + 1
    dst_rows = torch.arange(n, n + n_add, device=src_rows.device)
    _apply_relocation(p, m, v, ratio, dst_rows, src_rows, floor)
    return p, m, v
