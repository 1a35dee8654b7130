"""The training-step kernels behind the rasterizer against tests/train_ref64.py: k_adam (csrc/train_ops.hip,
csrc/adam_math.h), k_ssim_l1 / k_loss_finish (csrc/loss.hip), k_grad_stats (csrc/train_ops.hip).  The references, the
measures and the derivation of the bounds are in tests/train_ref64.py; tests/test_train_ref64.py holds them to
PyTorch's float64 results on the CPU and shows that correct fp32 implementations meet them.

Adam: every element of p', m', v' within (K + 1) 2^-24 abs_sum + 2^-126 of one float64 step from the kernel's own
inputs (K + 1 = 4 / 5 / 7 for m' / v' / p'; p' from the kernel's own m', v').
  launch shape   six tensors, 17 000 008 floats, one launch of more than 4 194 304 float4 chunks: the grid cap bites,
                 every thread of the first trip holds two chunks, a second trip runs; a group boundary inside the
                 first stride (pairs whose two chunks lie in different tensors), tail chunks and the scalar path of a
                 misaligned view in the second slot
  splitting      ten parameters -> launches of 8 and 2; other betas in the middle of the list -> three runs; grad None
  regimes        gradients log-uniform over 1e-30 .. 1e4 with zeros, m zero / random, v zero / denormal / ordinary /
                 1e8, steps 1 .. 1 000 000, eps 1e-8 and 1e-15, the six learning rates; 30 consecutive steps
  non-finite     NaN / +-inf gradients: the same non-finite elements as torch.optim.Adam (fp32, CPU)
Loss: ten shapes x six regimes (train_ref64.SHAPES, REGIMES), the gradient through r with the neighbourhood envelope
(bound 8), the scalars through their own bounds.
Densification statistics: bit-equal to the trainer's lines.
Every test also fails for a kernel that is subtly wrong: tests/test_train_ref64.py shows a dropped bias correction, a
wrong weight, a window column too many and a dropped gradient term far beyond the bounds.

Measured on an MI355X (nothing exceeded a bound; no kernel was changed):
  Adam, largest error in units of 2^-24 abs_sum, m' / v' / p' (bounds 4 / 5 / 7; torch.optim.Adam in fp32 on the CPU,
  same regimes: 1.8 / 1.9 / 4.2)
    launch shape (17 M floats)       2.61 / 2.89 / 3.05
    regimes, m zero                  0.95 / 2.69 / 2.99      (v 1e8: 0.95 / 0.89 / 1.00)
    regimes, m random                2.58 / 2.81 / 4.27      (p': v zero, eps 1e-15)
    30 consecutive steps             2.62 / 2.83 / 3.01
  Loss, largest value per regime over the ten shapes and ssim_frac 0 / 0.2 / 1: r of the gradient (bound 8; the
  separable fp32 restatement on the CPU: 1.14 at most), the SSIM error in units of mean|map32 - map64| beyond 2^-23
  (bound 8), and the l1 / mse / loss errors in units of their bounds (bound 1)
    noise            r 0.56   ssim 0.32   l1 0.32   mse 0.17   loss 0.12
    converged        r 0.92   ssim 0.22   l1 0.47   mse 0.13   loss 0.24
    bright_flat      r 0.38   ssim 0.16   l1 0.30   mse 0.22   loss 0.10
    out_of_range     r 0.73   ssim 0.08   l1 0.39   mse 0.11   loss 0.16
    zero_background  r 0.73   ssim 0.08   l1 0.37   mse 0.15   loss 0.18     (gradient exactly 0 far from the block)
    checkerboard     r 0.47   ssim 0.15   l1 0      mse 0      loss 0.04
  In absolute terms at 37x53, bright_flat: SSIM off by 4.1e-5, the loss by 1.0 %, the gradient by 1.7e-4 of its
  maximum (the fp32 2-D restatement: 4.5e-4, 10.8 %, 5.1e-4); converged: gradient 2.0e-5 of its maximum."""
import pytest
import torch

from gaussian_splatting_amd import _hip
from gaussian_splatting_amd.splat_py.structs import Camera
from gaussian_splatting_amd.train_ops import Adam, accumulate_grad_stats, ssim_l1_loss

from . import train_ref64 as T
from .helpers import report

pytestmark = pytest.mark.gpu
DEV = "cuda"
BETAS = (0.9, 0.999)
GRID_CAP, BLOCK = 8192, 256   # gs_adam_step (csrc/train_ops.hip)
STRIDE = GRID_CAP * BLOCK     # chunks per trip and slot once the cap bites


# ---- Adam ------------------------------------------------------------------------------------------------------------
class Tracked:
    """one parameter on the device with its gradient and preset (or absent) optimizer state, and CPU copies of all
    of them from before the step"""

    def __init__(self, p, g, m=None, v=None, step0=0, offset_view=False):
        self.n = p.numel()
        if offset_view:   # a view 4 bytes past a 16-byte boundary: the kernel's scalar path
            self.store = torch.cat((torch.full((1,), 123.0), p)).to(DEV)
            self.param = self.store[1:].detach().requires_grad_(True)
            assert self.param.data_ptr() % 16 == 4
        else:
            self.param = p.to(DEV).requires_grad_(True)
        self.param.grad = g.to(DEV)
        self.step0 = step0
        self.m = None if m is None else m.to(DEV)
        self.v = None if v is None else v.to(DEV)
        self.snapshot()

    def preset(self, opt):
        if self.m is not None:
            opt.state[self.param] = {"step": torch.tensor(float(self.step0)), "exp_avg": self.m, "exp_avg_sq": self.v}

    def snapshot(self):
        z = torch.zeros(self.n)
        self.before = (self.param.detach().cpu().clone(), self.param.grad.cpu().clone(),
                       z if self.m is None else self.m.cpu().clone(), z.clone() if self.v is None else self.v.cpu().clone())

    def scores(self, opt, lr, betas, eps):
        st = opt.state[self.param]
        self.step0 += 1
        assert float(st["step"]) == self.step0
        self.m, self.v = st["exp_avg"], st["exp_avg_sq"]
        after = (self.param.detach().cpu(), self.m.cpu(), self.v.cpu())
        return T.adam_scores(self.before, after, lr, self.step0, *betas, eps)


def spy_on_adam_launches(monkeypatch):
    """-> list that receives the numel tuple of every gs_adam_step launch"""
    launches, real = [], _hip.call

    def call(name, *args):
        if name == "gs_adam_step":
            launches.append(tuple(args[5][i] for i in range(args[0])))
        return real(name, *args)

    monkeypatch.setattr(_hip, "call", call)
    return launches


def test_adam_launch_shape_two_chunks_in_flight_and_a_second_trip(monkeypatch):
    sizes = (1_000_001, 9_000_003, 0, 5_000_001, 2_000_002, 1)
    VIEW = 4
    gen = torch.Generator().manual_seed(17)
    lr, eps = 0.004, 1e-15
    ts = []
    for i, n in enumerate(sizes):
        m, v = T.adam_state(n, gen, "random", "ordinary")
        ts.append(Tracked(torch.randn(n, generator=gen), T.adam_gradients(n, gen, lo=1e-12, hi=1e2), m, v,
                          step0=(0, 6, 0, 999, 29999, 1)[i], offset_view=(i == VIEW)))
    opt = Adam([t.param for t in ts], lr=lr, betas=BETAS, eps=eps)
    for t in ts:
        t.preset(opt)
    launches = spy_on_adam_launches(monkeypatch)
    opt.step()
    torch.cuda.synchronize()
    # what forces the paths, from the launch's own arguments
    assert launches == [sizes]
    ends, c = [], 0
    for n in sizes:
        c += (n + 3) // 4
        ends.append(c)
    total = ends[-1]
    assert total > 2 * STRIDE == 4_194_304          # the cap bites (`two` holds) and a second trip runs
    assert 0 < ends[0] < STRIDE                     # a group boundary strictly inside the first stride: pairs (c, c + STRIDE)
    assert ends[0] + STRIDE < ends[1]               # ... whose chunks lie in tensors 0 and 1, and beyond it both in 1
    assert STRIDE < ends[1] - 1 < 2 * STRIDE and sizes[1] % 4 != 0   # a tail chunk in the second slot
    assert STRIDE < ends[3] < 2 * STRIDE < ends[4]  # the misaligned view: second slot of trip one and the second trip
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for i, t in enumerate(ts):
        if t.n == 0:
            continue
        sc = t.scores(opt, lr, BETAS, eps)
        T.assert_adam_bounds(sc, f"tensor {i}")
        worst = {k: max(worst[k], sc[k]) for k in worst}
    assert float(ts[VIEW].store[0]) == 123.0        # the element in front of the offset view is untouched
    report("adam_ref64[launch shape]", **worst)


@pytest.mark.parametrize("layout", ["one_group", "betas_in_the_middle"])
def test_adam_step_splits_its_launches(monkeypatch, layout):
    gen = torch.Generator().manual_seed(23)
    sizes = [1001 + 37 * i for i in range(10)]
    ts = []
    for i, n in enumerate(sizes):
        fresh = i % 3 == 0
        m, v = (None, None) if fresh else T.adam_state(n, gen, "random", "ordinary")
        ts.append(Tracked(torch.randn(n, generator=gen), T.adam_gradients(n, gen, lo=1e-12, hi=1e2), m, v,
                          step0=0 if fresh else 10 * i))
    idle = torch.randn(77, generator=gen).to(DEV).requires_grad_(True)   # grad None: skipped, no state
    idle_before = idle.detach().clone()
    other = (0.8, 0.99)
    if layout == "one_group":
        groups = [{"params": [t.param for t in ts[:4]] + [idle] + [t.param for t in ts[4:]], "lr": 0.004}]
        hyper = [(0.004, BETAS)] * 10
        want = [tuple(sizes[:8]), tuple(sizes[8:])]
    else:
        groups = [{"params": [t.param for t in ts[:3]], "lr": T.LRS[0]},
                  {"params": [ts[3].param, idle, ts[4].param], "lr": T.LRS[2], "betas": other},
                  {"params": [t.param for t in ts[5:]], "lr": T.LRS[3]}]
        hyper = [(T.LRS[0], BETAS)] * 3 + [(T.LRS[2], other)] * 2 + [(T.LRS[3], BETAS)] * 5
        want = [tuple(sizes[:3]), tuple(sizes[3:5]), tuple(sizes[5:])]
    opt = Adam(groups, betas=BETAS, eps=1e-15)
    for t in ts:
        t.preset(opt)
    launches = spy_on_adam_launches(monkeypatch)
    opt.step()
    assert launches == want
    for i, t in enumerate(ts):
        T.assert_adam_bounds(t.scores(opt, hyper[i][0], hyper[i][1], 1e-15), f"tensor {i}")
    assert len(opt.state[idle]) == 0 and torch.equal(idle.detach(), idle_before)


@pytest.mark.parametrize("m_kind", T.M_KINDS)
@pytest.mark.parametrize("v_kind", T.V_KINDS)
def test_adam_regimes(m_kind, v_kind):
    n = 100_003
    gen = torch.Generator().manual_seed(31 + 7 * T.M_KINDS.index(m_kind) + T.V_KINDS.index(v_kind))
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for i, (step, eps) in enumerate((s, e) for s in T.STEPS for e in T.EPSS):
        lr = T.LRS[(i + T.V_KINDS.index(v_kind)) % len(T.LRS)]
        m, v = T.adam_state(n, gen, m_kind, v_kind)
        t = Tracked(torch.randn(n, generator=gen), T.adam_gradients(n, gen), m, v, step0=step - 1)
        opt = Adam([t.param], lr=lr, betas=BETAS, eps=eps)
        t.preset(opt)
        opt.step()
        sc = t.scores(opt, lr, BETAS, eps)
        T.assert_adam_bounds(sc, (step, eps, lr))
        worst = {k: max(worst[k], sc[k]) for k in worst}
    report(f"adam_ref64[regimes m {m_kind}, v {v_kind}]", **worst)


def test_adam_thirty_consecutive_steps():
    """each step checked from the kernel's own previous state: one tensor deep into training, one freshly reset (no
    state: the case after reset_opacity)"""
    n, lr, eps = 100_003, T.LRS[3], 1e-15
    gen = torch.Generator().manual_seed(41)
    m, v = T.adam_state(n, gen, "random", "ordinary")
    old = Tracked(torch.randn(n, generator=gen), T.adam_gradients(n, gen), m, v, step0=29_990)
    new = Tracked(torch.randn(n, generator=gen), T.adam_gradients(n, gen))
    opt = Adam([old.param, new.param], lr=lr, betas=BETAS, eps=eps)
    old.preset(opt)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for it in range(30):
        for t in (old, new):
            if it:
                t.param.grad = T.adam_gradients(n, gen).to(DEV)
                t.snapshot()
        opt.step()
        for t in (old, new):
            sc = t.scores(opt, lr, BETAS, eps)
            T.assert_adam_bounds(sc, it)
            worst = {k: max(worst[k], sc[k]) for k in worst}
    assert old.step0 == 30_020 and new.step0 == 30
    report("adam_ref64[30 steps]", **worst)


def test_adam_non_finite_gradients_spread_as_in_torch():
    n, lr, eps, step = 10_007, 0.004, 1e-8, 5
    gen = torch.Generator().manual_seed(43)
    p, g = torch.randn(n, generator=gen), T.adam_gradients(n, gen, lo=1e-12, hi=1e2)
    m, v = T.adam_state(n, gen, "random", "ordinary")
    for i, bad in zip((0, 3, 255, 256, 4097, n - 2, n - 1), (float("nan"), float("inf"), -float("inf")) * 3):
        g[i] = bad
    t = Tracked(p, g, m, v, step0=step - 1)
    opt = Adam([t.param], lr=lr, betas=BETAS, eps=eps)
    t.preset(opt)
    opt.step()
    sc = t.scores(opt, lr, BETAS, eps)
    q = p.clone().requires_grad_(True)
    q.grad = g.clone()
    ref = torch.optim.Adam([q], lr=lr, betas=BETAS, eps=eps)
    ref.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    ref.step()
    for got, want in zip(sc["nonfinite"], (q.detach(), ref.state[q]["exp_avg"], ref.state[q]["exp_avg_sq"])):
        assert int(got.sum()) == 7 and torch.equal(got, ~torch.isfinite(want))
    T.assert_adam_bounds(sc)   # every other element


# ---- loss ------------------------------------------------------------------------------------------------------------
LOSS_CASES = [(r, H, W, 0.2) for r in T.REGIMES for H, W in T.SHAPES] + \
             [(r, H, W, f) for r in T.REGIMES for H, W in ((17, 33), (37, 53)) for f in (0.0, 1.0)]


@pytest.mark.parametrize("regime,H,W,frac", LOSS_CASES)
def test_ssim_l1_loss_against_float64(regime, H, W, frac):
    case = T.loss_reference(regime, H, W, frac)
    img = case["image"].to(DEV).requires_grad_(True)
    tgt = case["target"].to(DEV)
    loss, terms = ssim_l1_loss(img, tgt, frac, return_terms=True)
    loss.backward()
    grad, tm = img.grad.cpu(), [float(x) for x in terms.cpu()]
    assert float(loss.detach()) == tm[0]
    sc = T.loss_scores(case, T.R_MAX, tm[0], tm[1], tm[2], tm[3], grad)
    report(f"loss_ref64[{regime}, {H}x{W}, ssim_frac {frac}]", **sc)
    T.assert_loss_bounds(sc, T.R_MAX, (regime, H, W, frac))
    if regime == "zero_background":
        assert not bool(grad[T.far_from_block(H, W)].any())
    # a power-of-two upstream gradient scales the gradient exactly
    img4 = case["image"].to(DEV).requires_grad_(True)
    (4.0 * ssim_l1_loss(img4, tgt, frac)).backward()
    assert torch.equal(img4.grad.cpu(), 4.0 * grad)
    # without requires_grad (no gradient written): the same terms, bit for bit
    _, terms_plain = ssim_l1_loss(case["image"].to(DEV), tgt, frac, return_terms=True)
    assert torch.equal(terms_plain, terms)


# ---- densification statistics ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("culled", ["all", "none", "some"])
@pytest.mark.parametrize("layout", ["contiguous", "slab_view"])
def test_accumulate_grad_stats_equals_the_trainer_lines(N, culled, layout):
    gen = torch.Generator().manual_seed(N * 7 + len(culled))
    K = torch.tensor([[311.5, 0.0, 160.0], [0.0, 287.25, 120.0], [0.0, 0.0, 1.0]])   # fx != fy
    cam = Camera(320, 240, K.to(DEV))
    mask = {"all": torch.ones(N, dtype=torch.bool), "none": torch.zeros(N, dtype=torch.bool),
            "some": torch.rand(N, generator=gen) < 0.3}[culled].to(DEV)
    V = int((~mask).sum())
    slab = torch.randn(V, 9, generator=gen)             # both signs
    slab[::3, 4] = 0.0                                  # exact zeros
    slab[1::4, 5] = -0.0
    slab = slab.to(DEV)
    uv_grad = slab[:, 4:6] if layout == "slab_view" else slab[:, 4:6].contiguous()
    xyz_grad = torch.randn(N, 3, generator=gen)
    xyz_grad[::5] = 0.0
    xyz_grad = xyz_grad.to(DEV)
    uv_acc = torch.rand(N, 2, generator=gen).to(DEV)
    xyz_acc = torch.rand(N, 3, generator=gen).to(DEV)
    count = torch.randint(0, 5, (N,), generator=gen, dtype=torch.int32).to(DEV)   # counts that start non-zero
    # trainer.py:378-385, literally
    ref_uv, ref_xyz, ref_count = uv_acc.clone(), xyz_acc.clone(), count.clone()
    ug = uv_grad.detach().clone()
    ug[:, 0] = ug[:, 0] * cam.K[0, 0]
    ug[:, 1] = ug[:, 1] * cam.K[1, 1]
    ref_uv[~mask] += torch.abs(ug)
    ref_xyz += torch.abs(xyz_grad)
    ref_count += (~mask).int()
    before, uv_before = slab.clone(), uv_grad.clone()
    accumulate_grad_stats(uv_grad, mask, xyz_grad, cam, uv_acc, xyz_acc, count)
    assert torch.equal(uv_acc, ref_uv) and torch.equal(xyz_acc, ref_xyz) and torch.equal(count, ref_count)
    assert torch.equal(slab, before) and torch.equal(uv_grad, uv_before)
