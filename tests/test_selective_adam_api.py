"""train_ops.SelectiveAdam and gs_adam_step_rows where their callers look for them, and the optimizer's semantics on
CPU tensors (no GPU needed): the header declares the entry point, the built library exports it at ABI 13 with the
header's prototype; step(culling_mask=...) on fp32 CPU tensors goes through torch's functional Adam on the visible
rows and leaves every bit of a culled row alone; without a mask it is train_ops.Adam.step; bad masks, shapes and
unsupported groups are refused before any state changes."""
import ctypes
import os
import re

import pytest
import torch

from gaussian_splatting_amd import _hip
from gaussian_splatting_amd.train_ops import Adam, SelectiveAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (3, 4, 3, 1, 3, 45)   # xyz, quaternion, scale, opacity, rgb, sh at degree 3
LRS = (0.0002, 0.004, 0.01, 0.02, 0.004, 0.0002)
N = 37
ODD = (float("nan"), float("inf"), float("-inf"), 1e-41)   # 1e-41: a denormal


def test_header_declares_and_library_exports_the_entry_point():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+gs_adam_step_rows\s*\(", src)
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "gs_adam_step_rows")
    assert "gs_adam_step_rows" in _hip.EXPORTS
    lib = _hip.lib()
    fn = lib.gs_adam_step_rows
    P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    # n_groups | params grads exp_avg exp_avg_sq numel row_width skip_row | n_rows | lr step | beta1 beta2 eps | stream
    assert fn.restype is I and list(fn.argtypes) == [I] + [P] * 7 + [L] + [P] * 2 + [D] * 3 + [P]
    assert lib.gs_abi_version() >= 13


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def tensors(gen, n=N):
    return [torch.randn(n, w, generator=gen).requires_grad_(True) for w in WIDTHS]


def groups(ps):
    return [{"params": [p], "lr": lr} for p, lr in zip(ps, LRS)]


def test_masked_steps_match_dense_adam_on_visible_rows_and_leave_culled_rows_alone():
    gen = torch.Generator().manual_seed(41)
    ps = tensors(gen)
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    sel, ref = SelectiveAdam(groups(ps)), torch.optim.Adam(groups(qs))
    for it in range(5):
        culled = torch.rand(N, generator=gen) < (0.2, 0.5, 0.8, 0.5, 0.35)[it]
        culled[it], culled[N - 1 - it] = True, False   # at least one of each
        rows = culled.nonzero().squeeze(1)
        for p, q in zip(ps, qs):
            grad = torch.randn(p.shape, generator=gen) * 10.0 ** (it % 3 - 2)
            p.grad, q.grad = grad.clone(), grad.clone()
            # NaN, +-inf and a denormal in the culled rows of p, both moments and the gradient, in both copies
            odd = torch.tensor(ODD)[torch.randint(0, 4, (len(rows), p.shape[1]), generator=gen)]
            fresh = torch.randn(3, *p.shape, generator=gen)   # what a row culled before wakes up with
            with torch.no_grad():
                for opt, t in ((sel, p), (ref, q)):
                    if it:
                        t[was_culled] = fresh[0][was_culled]
                        opt.state[t]["exp_avg"][was_culled] = 0.1 * fresh[1][was_culled]
                        opt.state[t]["exp_avg_sq"][was_culled] = 0.01 * fresh[2][was_culled].abs()
                    t[rows] = odd
                    t.grad[rows] = odd.flip(0)
                    if opt.state[t]:
                        opt.state[t]["exp_avg"][rows] = odd.flip(1)
                        opt.state[t]["exp_avg_sq"][rows] = odd.abs()
        before = [(q.detach().clone(), *(ref.state[q][k].clone() if ref.state[q] else torch.zeros_like(q)
                                         for k in ("exp_avg", "exp_avg_sq"))) for q in qs]
        held = [(bits(p).clone(), *(bits(sel.state[p][k]).clone() if sel.state[p] else bits(torch.zeros_like(p))
                                    for k in ("exp_avg", "exp_avg_sq"))) for p in ps]
        sel.step(culling_mask=culled)
        ref.step()
        for i, (p, q) in enumerate(zip(ps, qs)):
            with torch.no_grad():   # the dense reference: its culled rows go back to their values from before the step
                q[rows] = before[i][0][rows]
                ref.state[q]["exp_avg"][rows] = before[i][1][rows]
                ref.state[q]["exp_avg_sq"][rows] = before[i][2][rows]
            got = (p.detach(), sel.state[p]["exp_avg"], sel.state[p]["exp_avg_sq"])
            want = (q.detach(), ref.state[q]["exp_avg"], ref.state[q]["exp_avg_sq"])
            for name, a, b, h in zip(("param", "exp_avg", "exp_avg_sq"), got, want, held[i]):
                assert torch.equal(bits(a)[rows], h[rows]), (it, i, name)            # culled: bit patterns
                err = (a[~culled] - b[~culled]).abs().max() / b[~culled].abs().max()
                assert float(err) < 2e-6, (it, i, name, float(err))                    # visible: a few ulp
                assert torch.isfinite(a[~culled]).all()
        was_culled = rows
    for p, q in zip(ps, qs):
        assert float(sel.state[p]["step"]) == float(ref.state[q]["step"]) == 5


def test_no_mask_is_adam_step():
    gen = torch.Generator().manual_seed(43)
    ps = tensors(gen)
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    sel, ref = SelectiveAdam(groups(ps)), Adam(groups(qs))
    for it in range(3):
        for p, q in zip(ps, qs):
            p.grad = torch.randn(p.shape, generator=gen)
            q.grad = p.grad.clone()
        sel.step(culling_mask=None) if it else sel.step()
        ref.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q) and float(sel.state[p]["step"]) == 3
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sel.state[p][k], ref.state[q][k])


def snapshot(opt):
    return {id(p): {k: v.clone() for k, v in opt.state[p].items()} | {"p": p.detach().clone()}
            for g in opt.param_groups for p in g["params"]}


def unchanged(opt, snap):
    for g in opt.param_groups:
        for p in g["params"]:
            was = snap[id(p)]
            if not torch.equal(bits(p), bits(was["p"])) or set(opt.state[p]) != set(was) - {"p"}:
                return False
            if any(not torch.equal(opt.state[p][k], was[k]) for k in opt.state[p]):
                return False
    return True


def stepped_once(step=True, **extra):
    gen = torch.Generator().manual_seed(47)
    ps = tensors(gen)
    opt = SelectiveAdam(groups(ps), **extra)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen)
    if step:
        opt.step()
    return opt, ps


@pytest.mark.parametrize("mask,match", [
    (torch.zeros(N, dtype=torch.uint8), "1-D bool"),
    (torch.zeros(N, 1, dtype=torch.bool), "1-D bool"),
    ([False] * N, "1-D bool"),
    (torch.zeros(N, dtype=torch.bool, device="meta"), "culling_mask is on meta"),
    (torch.zeros(N + 1, dtype=torch.bool), r"parameter 0 of group 0 has shape \(37, 3\), culling_mask 38 rows"),
])
def test_bad_masks_raise_value_error_before_any_state_changes(mask, match):
    for fresh in (True, False):
        if fresh:
            ps = tensors(torch.Generator().manual_seed(47))
            opt = SelectiveAdam(groups(ps))
            for p in ps:
                p.grad = torch.ones_like(p)
        else:
            opt, ps = stepped_once()
        snap = snapshot(opt)
        with pytest.raises(ValueError, match=match):
            opt.step(culling_mask=mask)
        assert unchanged(opt, snap)
        assert all(len(opt.state[p]) == 0 for p in ps) if fresh else all(float(opt.state[p]["step"]) == 1 for p in ps)


def test_one_parameter_of_another_height_is_named():
    opt, ps = stepped_once()
    odd = torch.randn(N + 2, 3, requires_grad=True)
    odd.grad = torch.ones_like(odd)
    opt.add_param_group({"params": [odd], "lr": 0.1})
    snap = snapshot(opt)
    with pytest.raises(ValueError, match="parameter 0 of group 6"):
        opt.step(culling_mask=torch.zeros(N, dtype=torch.bool))
    assert unchanged(opt, snap)
    odd.grad = None   # without a gradient it is not stepped, so its height does not matter
    opt.step(culling_mask=torch.zeros(N, dtype=torch.bool))
    assert all(float(opt.state[p]["step"]) == 2 for p in ps) and len(opt.state[odd]) == 0


@pytest.mark.parametrize("extra", [dict(amsgrad=True), dict(weight_decay=0.01), dict(maximize=True),
                                   dict(capturable=True), dict(differentiable=True)])
def test_unsupported_groups_raise_with_a_mask_and_step_as_adam_without(extra):
    name = next(iter(extra))
    # without a mask: Adam.step, which hands these to torch (whose capturable / differentiable steps do not run on
    # CPU leaves: those two start from an optimizer without state)
    runs_on_cpu = name not in ("capturable", "differentiable")
    opt, ps = stepped_once(step=runs_on_cpu, **extra)
    assert all(float(opt.state[p]["step"]) == 1 if runs_on_cpu else len(opt.state[p]) == 0 for p in ps)
    snap = snapshot(opt)
    with pytest.raises(RuntimeError, match=f"{name} in param group 0"):
        opt.step(culling_mask=torch.zeros(N, dtype=torch.bool))
    assert unchanged(opt, snap)


def test_all_true_mask_changes_nothing_but_step():
    opt, ps = stepped_once()
    snap = snapshot(opt)
    fresh = torch.randn(N, 2, requires_grad=True)   # no state yet: it gets zero moments and step 1
    fresh.grad = torch.ones_like(fresh)
    opt.add_param_group({"params": [fresh], "lr": 0.1})
    for p in ps:
        p.grad = torch.full_like(p, float("nan"))   # not read
    opt.step(culling_mask=torch.ones(N, dtype=torch.bool))
    for p in ps:
        was = snap[id(p)]
        assert torch.equal(p, was["p"]) and float(opt.state[p]["step"]) == 2
        assert torch.equal(opt.state[p]["exp_avg"], was["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], was["exp_avg_sq"])
    st = opt.state[fresh]
    assert float(st["step"]) == 1 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
