"""MCMC densification without a GPU: the float64 relocation reference (tests/mcmc_ref.py) against 80-digit arithmetic,
the identities the kernel relies on, the clamps, the two entry points where their callers look for them (header,
library, _hip, ABI 17) and the controller's refusals by name."""
import ctypes
import math
import os
import re

import pytest
import torch

from gaussian_splatting_amd import _hip
from gaussian_splatting_amd.densify import MCMCConfig, MCMCController
from gaussian_splatting_amd.synthetic import make_scene

from . import mcmc_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPACITIES = (0.005, 0.1, 0.5, 0.9, 0.99, 0.999, 0.9999, 1 - 2.0 ** -20, 1 - 2.0 ** -24)
RATIOS = (2, 3, 5, 10, 20, 51)
PROTOTYPES = {
    "gs_mcmc_relocate":
        "int n_tensors, void* const* params, void* const* exp_avg, void* const* exp_avg_sq, const int32_t* width, "
        "const int32_t* kind, int n_rows, const int32_t* ratio, const int32_t* dst_rows, const int32_t* src_rows, int M, "
        "float min_opacity, void* stream",
    "gs_mcmc_add_noise":
        "void* xyz, const void* quaternion, const void* scale, const void* opacity, const void* noise, int N, float step, "
        "float gate_k, float gate_x0, void* stream",
}


def test_float64_reference_against_80_digits():
    """o_new and the published double sum in float64 against mpmath at 80 digits, from the same float64 o: the relative
    error of denom (and of o_new) is at most 1e-11 on the whole grid"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 80
    worst = 0.0
    for o in OPACITIES:
        for n in RATIOS:
            o64 = torch.tensor([o], dtype=torch.float64)
            o_new = M.opacity_new(o64, n)
            denom = M.denom_double_sum(o_new, n)
            eo = 1 - (1 - mp.mpf(o)) ** (mp.mpf(1) / n)
            ed = mp.mpf(0)
            for i in range(1, n + 1):
                for k in range(i):
                    ed += mp.binomial(i - 1, k) * (-1) ** k * eo ** (k + 1) / mp.sqrt(k + 1)
            err_o = abs((mp.mpf(float(o_new)) - eo) / eo)
            err_d = abs((mp.mpf(float(denom)) - ed) / ed)
            worst = max(worst, float(err_d))
            assert err_o <= 1e-11 and err_d <= 1e-11, (o, n, float(err_o), float(err_d))
    print("worst relative error of denom: %.3g" % worst)


def test_identities():
    for o in OPACITIES:
        for n in RATIOS:
            o64 = torch.tensor([o], dtype=torch.float64)
            o_new = M.opacity_new(o64, n)
            a, b = M.denom_double_sum(o_new, n), M.denom_hockey_stick(o_new, n)
            assert abs(float(a - b)) <= 1e-11 * abs(float(a)), (o, n, float(a), float(b))      # hockey stick
            back = 1.0 - (1.0 - o_new) ** n
            assert abs(float(back) - o) <= 1e-12 * n, (o, n, float(back))        # n copies composite to o again
            assert float(torch.log(o64 / a)) < 0.0, (o, n)                       # every copy is smaller than its source
            assert float(torch.log(o64 / b)) < 0.0, (o, n)
    # the binomials of the kernel's recurrence C(n,k+1) = C(n,k) (n-k) / (k+1) are exact in double up to n = 51
    for n in (2, 20, M.MAX_RATIO):
        c = 1.0
        for k in range(n):
            assert c * (n - k) < 2.0 ** 53
            c = c * (n - k) / (k + 1)
            assert c == math.comb(n, k + 1)


def test_relocation_clamps():
    x = torch.tensor([0.3, 0.3, 0.3, 30.0, 30.0], dtype=torch.float32)
    ratio = torch.tensor([51, 52, 1000, 2, 2])
    logit, shift, o_new, denom = M.relocation(x, ratio, 0.005)
    assert float(logit[0]) == float(logit[1]) == float(logit[2]) and float(shift[0]) == float(shift[2])   # ratio at 51
    # sigmoid(30) is 1 - 9e-14: the clamp makes it 1 - 2^-24, whose square root of the rest is 2^-12
    assert abs(float(o_new[3]) - (1.0 - 2.0 ** -12)) < 1e-12 and bool(torch.isfinite(shift).all())
    ref = M.relocation(torch.tensor([math.log(M.O_MAX / (1 - M.O_MAX))], dtype=torch.float64).float(), ratio[3:4], 0.005)
    assert abs(float(ref[2]) - float(o_new[3])) < 1e-9
    # min_opacity (the fp32 value the C ABI carries) floors the new opacity, not the scale correction
    low = M.relocation(torch.tensor([-5.0]), torch.tensor([10]), 0.005)
    floor = float(torch.tensor(0.005, dtype=torch.float32))
    assert abs(float(low[0]) - math.log(floor / (1.0 - floor))) < 1e-12 and float(low[2]) < 0.005
    assert abs(float(low[1]) - float(M.relocation(torch.tensor([-5.0]), torch.tensor([10]), 1e-6)[1])) == 0.0


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert re.search(r"^#define GS_MCMC_MAX_RATIO 51\s", src, flags=re.M)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    lib = _hip.lib()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = {"gs_mcmc_relocate": [I] + [P] * 5 + [I] + [P] * 3 + [I, F, P],
            "gs_mcmc_add_noise": [P] * 5 + [I] + [F] * 3 + [P]}
    for n, args in PROTOTYPES.items():
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % n, src)
        assert found, n
        assert " ".join(found.group(1).split()).replace(" ,", ",") == args, n   # (the [n_rows] / [M] / [N,3] notes are comments)
        assert hasattr(raw, n), n
        assert n in _hip.EXPORTS
        fn = getattr(lib, n)
        assert fn.restype is I and list(fn.argtypes) == want[n], n   # typed from the header, no hand wrapper
    assert _hip.GS_MCMC_MAX_RATIO == 51 == M.MAX_RATIO
    assert lib.gs_abi_version() >= 17


def test_controller_refuses_by_name():
    class NoOptimizer:
        param_groups, state = [], {}

    g, _, _ = make_scene(50, 32, 32, 0, seed=1, device="cpu")
    ctrl = MCMCController(g, NoOptimizer(), MCMCConfig())
    for call in (ctrl.relocate, ctrl.add_new, lambda: ctrl.inject_noise(1e-4), lambda: ctrl.step(600, 1e-4)):
        with pytest.raises(RuntimeError, match="needs float32 tensors on the GPU"):
            call()
    ctrl = MCMCController(g, NoOptimizer(), MCMCConfig(cap_max=49))
    for call in (ctrl.relocate, ctrl.add_new):
        with pytest.raises(RuntimeError, match="cap_max 49 is below the current count 50"):
            call()
    # more rows than torch.multinomial takes (stride-0 views: the guard reads the row count before anything else)
    big = lambda w: torch.zeros(1, w).expand((1 << 24) + 1, w)
    ctrl.gaussians = type(g)(big(3), big(3), big(1), big(3), big(4), None)
    with pytest.raises(RuntimeError, match="16777217 Gaussians are more than 2\\^24, the limit of torch.multinomial"):
        ctrl.relocate()
    cfg = MCMCConfig()
    assert (cfg.cap_max, cfg.min_opacity, cfg.grow_factor, cfg.noise_lr, cfg.gate_k, cfg.gate_x0) == \
        (1_000_000, 0.005, 1.05, 5e5, 100.0, 0.995)
    assert (cfg.refine_start, cfg.refine_stop, cfg.refine_every, cfg.opacity_reg, cfg.scale_reg) == \
        (500, 25_000, 100, 0.01, 0.01)
