"""The antialiased opacity (GS_RASTER_ANTIALIASED, include/gsplat_hip.h "antialiased opacity") written from its formula
(test code only).

  Sigma2D = [[conic0, conic1 / 2], [conic1 / 2, conic2]]
  comp    = sqrt(det Sigma2D / det(Sigma2D + 0.25 I))   where both determinants are positive, else 0
  opa_eff = opacity_act * comp

opacity_eff_fp64 is that, in float64 with torch autograd.  aa_terms / fold_slab evaluate the header's expressions in a
given dtype, in the header's order (what the kernels do in fp32: torch's CPU elementwise operations are IEEE and not
contracted)."""
import torch


def opacity_eff_fp64(conic, opacity_act):
    """conic [V,3], opacity_act [V,1] (float64, may require grad) -> opa_eff [V,1]"""
    assert conic.dtype == torch.float64 and opacity_act.dtype == torch.float64
    s00, s01, s11 = conic[:, 0], conic[:, 1] / 2, conic[:, 2]
    det_0 = s00 * s11 - s01 * s01
    det_d = (s00 + 0.25) * (s11 + 0.25) - s01 * s01
    with torch.no_grad():
        ok = (det_0 > 0) & (det_d > 0)
    # (the unselected branch of a where() must not carry a NaN into the derivative: take the root of 1 there)
    rho = torch.where(ok, det_0 / torch.where(ok, det_d, torch.ones_like(det_d)), torch.ones_like(det_0))
    comp = torch.where(ok, torch.sqrt(rho), torch.zeros_like(rho))
    return opacity_act * comp[:, None]


def aa_terms(conic, dtype):
    """the header's a0, c0, b, a, c, det_0, det_d, comp of conic [V,3], evaluated in dtype, in its order"""
    conic = conic.detach().to(dtype)
    a0, c0 = conic[:, 0], conic[:, 2]
    b = conic[:, 1] * 0.5
    a = a0 + 0.25
    c = c0 + 0.25
    det_d = a * c - b * b
    det_0 = a0 * c0 - b * b
    rho = det_0 / det_d
    ok = (det_0 > 0) & (det_d > 0)
    comp = torch.where(ok, torch.sqrt(torch.where(ok, rho, torch.ones_like(rho))), torch.zeros_like(rho))
    return dict(a0=a0, c0=c0, b=b, a=a, c=c, det_0=det_0, det_d=det_d, comp=comp)


def opacity_eff(conic, opacity_act, dtype):
    """opa_eff [V,1] = opacity_act * comp evaluated in dtype"""
    return opacity_act.detach().to(dtype).reshape(-1, 1) * aa_terms(conic, dtype)["comp"][:, None]


def fold_slab(conic, opacity_act, slab, dtype):
    """The backward of opa_eff folded into the render-gradient slab [V,9] (rgb 3 | opacity 1 | uv 2 | conic 3), whose
    column 3 is dL/d opa_eff: -> the slab of the classic chain (column 3 = dL/d opacity_act, the conic columns with the
    factor's terms added), evaluated in dtype in the header's order"""
    t = aa_terms(conic, dtype)
    y = opacity_act.detach().to(dtype).reshape(-1)
    out = slab.detach().to(dtype).clone()
    g = out[:, 3].clone()
    comp, det_0, det_d = t["comp"], t["det_0"], t["det_d"]
    out[:, 3] = g * comp
    pos = comp > 0
    safe = torch.where(pos, comp, torch.ones_like(comp))
    g_rho = g * y * 0.5 / safe
    dd = det_d * det_d
    zero = torch.zeros_like(g)
    out[:, 6] += torch.where(pos, g_rho * (t["c0"] * det_d - det_0 * t["c"]) / dd, zero)
    out[:, 7] += torch.where(pos, g_rho * t["b"] * (det_0 - det_d) / dd, zero)
    out[:, 8] += torch.where(pos, g_rho * (t["a0"] * det_d - det_0 * t["a"]) / dd, zero)
    return out
