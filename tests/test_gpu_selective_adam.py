"""train_ops.SelectiveAdam / gs_adam_step_rows (k_adam_rows, csrc/train_ops.hip) on the GPU.

The reference is the dense kernel itself: train_ops.Adam.step() on a second copy of the tensors, after which the rows
the mask culls are put back to their values from before the step.  The selective step must equal that under
torch.equal -- the same adam_update on the same inputs gives the same bits -- and must leave every bit of a culled row
alone, whatever it holds.

  bit equality     six tensors of widths 3, 4, 3, 1, 3, 45 (chunks that straddle up to four rows, a tail per tensor at
                   N = 1003), one of them a view 4 bytes past a 16-byte boundary (scalar path), a different
                   state["step"] per tensor, seven kinds of mask, ten steps
  culled rows      NaN, +-inf and denormals in the culled rows of p, m, v and the gradient come out bit-identical,
                   visible rows finite, a sentinel behind (and, for the view, in front of) every storage unchanged
  launch paths     17.7 M elements in one launch: the grid cap bites, a second trip runs, a group boundary inside the
                   first stride; and one tensor of more than 2^31 elements (64-bit row index)
  splitting        ten tensors -> launches of 8 and 2; other betas in the middle -> three
  surgery          the reference's delete / add on the optimizer state between masked steps
  end to end       the small training loop with the frame's own culling mask"""
import pytest
import torch

from gaussian_splatting_amd import _hip
from gaussian_splatting_amd.synthetic import make_scene
from gaussian_splatting_amd.train_ops import Adam, SelectiveAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("xyz", "quaternion", "scale", "opacity", "rgb", "sh")
WIDTHS = (3, 4, 3, 1, 3, 45)   # at degree 3
LRS = (0.0002, 0.004, 0.01, 0.02, 0.004, 0.0002)   # the reference's config.py: base_lr 0.002 times the multipliers
STEP0 = (0, 6, 0, 999, 29999, 1)   # as after an opacity reset: the counts differ between tensors
VIEW = 2                           # this tensor is an offset view
GRID_CAP, BLOCK = 8192, 256        # gs_adam_step_rows (csrc/train_ops.hip): k_adam's launch constants
STRIDE = GRID_CAP * BLOCK          # chunks per trip and slot once the cap bites
FRONT, BEHIND = 123.0, 456.0


def bits(t):
    return t.detach().contiguous().view(torch.int32)


class Slab:
    """a [n, w] tensor that is a view into a storage with a sentinel element behind it and, with lead=1, one in front
    (the view then starts 4 bytes past a 16-byte boundary)"""

    def __init__(self, values, lead=0):
        n = values.numel()
        self.store = torch.empty(lead + n + 1, device=DEV)
        self.store[:lead] = FRONT
        self.store[lead + n:] = BEHIND
        self.lead = lead
        self.view = self.store[lead:lead + n].view(values.shape)
        self.view.copy_(values)
        assert self.view.data_ptr() % 16 == 4 * lead

    def intact(self):
        return bool((self.store[:self.lead] == FRONT).all()) and float(self.store[-1]) == BEHIND


class Twin:
    """the tensors twice, with equal preset optimizer state: `sel` takes masked steps, `ref` dense Adam steps whose
    culled rows are put back"""

    def __init__(self, n, widths=WIDTHS, lrs=LRS, step0=STEP0, view=VIEW, seed=0, groups=None, device_rand=False):
        gen = torch.Generator(device=DEV if device_rand else "cpu").manual_seed(seed)
        self.gen, self.n, self.rand_dev = gen, n, DEV if device_rand else "cpu"
        self.slabs, self.p, self.q, states = [], [], [], []
        for i, w in enumerate(widths):
            p0 = self.randn(n, w)
            m0, v0 = 0.1 * self.randn(n, w), 0.01 * self.randn(n, w).abs()
            sp, sm, sv = Slab(p0, lead=int(i == view)), Slab(m0), Slab(v0)
            self.slabs += [sp, sm, sv]
            self.p.append(sp.view.detach().requires_grad_(True))
            self.q.append(p0.to(DEV).clone().requires_grad_(True))
            states.append((sm.view, sv.view, m0.to(DEV).clone(), v0.to(DEV).clone()))
        mk = groups or (lambda ts: [{"params": [t], "lr": lr} for t, lr in zip(ts, lrs)])
        self.sel, self.ref = SelectiveAdam(mk(self.p)), Adam(mk(self.q))
        for i, (p, q) in enumerate(zip(self.p, self.q)):
            if step0[i] is None:   # no state yet: both optimizers create it
                continue
            self.sel.state[p] = {"step": torch.tensor(float(step0[i])), "exp_avg": states[i][0], "exp_avg_sq": states[i][1]}
            self.ref.state[q] = {"step": torch.tensor(float(step0[i])), "exp_avg": states[i][2], "exp_avg_sq": states[i][3]}

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.gen, device=self.rand_dev)

    def set_grads(self, scale=1.0):
        for p, q in zip(self.p, self.q):
            g = (scale * self.randn(*p.shape)).to(DEV)
            p.grad, q.grad = g, g.clone()

    def triples(self, opt, ts):
        return [(t.detach(), opt.state[t]["exp_avg"], opt.state[t]["exp_avg_sq"]) for t in ts]

    def step_and_compare(self, culled, where=""):
        rows = culled.nonzero().squeeze(1)
        before = []
        for q in self.q:   # a tensor without state yet starts from zero moments
            st = self.ref.state[q]
            before.append((q.detach()[rows].clone(),
                           st["exp_avg"][rows].clone() if st else torch.zeros_like(q.detach()[rows]),
                           st["exp_avg_sq"][rows].clone() if st else torch.zeros_like(q.detach()[rows])))
        self.ref.step()
        with torch.no_grad():
            for tr, was in zip(self.triples(self.ref, self.q), before):
                for t, b in zip(tr, was):
                    t[rows] = b
        self.sel.step(culling_mask=culled)
        for i, (a, b) in enumerate(zip(self.triples(self.sel, self.p), self.triples(self.ref, self.q))):
            for name, x, y in zip(("param", "exp_avg", "exp_avg_sq"), a, b):
                assert torch.equal(x, y), (where, i, name, int((x != y).sum()))
            assert float(self.sel.state[self.p[i]]["step"]) == float(self.ref.state[self.q[i]]["step"])
        assert all(s.intact() for s in self.slabs), where


MASKS = ("none_culled", "all_culled", "row0_visible", "last_row_visible", "alternating", "random_10pc_visible",
         "visible_block")


def make_mask(kind, n, it, gen):
    culled = torch.ones(n, dtype=torch.bool)
    if kind == "none_culled":
        culled[:] = False
    elif kind == "row0_visible":
        culled[0] = False
    elif kind == "last_row_visible":
        culled[n - 1] = False
    elif kind == "alternating":
        culled[it % 2::2] = False
    elif kind == "random_10pc_visible":
        culled = torch.rand(n, generator=gen) >= 0.1
    elif kind == "visible_block":
        a = int(torch.randint(0, n, (1,), generator=gen))
        culled[a:a + max(1, n // 3)] = False
    return culled.to(DEV)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", [1, 5, 1003])
def test_masked_step_is_the_dense_step_on_the_visible_rows(n, kind):
    tw = Twin(n, seed=n)
    gen = torch.Generator().manual_seed(100 + n)
    for it in range(10):
        tw.set_grads(10.0 ** (it % 3 - 2))
        tw.step_and_compare(make_mask(kind, n, it, gen), where=f"step {it}")
    for i, p in enumerate(tw.p):
        assert float(tw.sel.state[p]["step"]) == STEP0[i] + 10   # whatever the masks said
    assert tw.p[VIEW].data_ptr() % 16 == 4   # the scalar path ran; step_and_compare checked the element in front


def test_culled_rows_are_not_touched_whatever_they_hold():
    n = 1003
    tw = Twin(n, seed=7)
    gen = torch.Generator().manual_seed(8)
    odd = torch.tensor([float("nan"), float("inf"), float("-inf"), 1e-41, -3e-45]).to(DEV)
    nan_payload = torch.tensor([0x7FC12345], dtype=torch.int32).view(torch.float32).to(DEV)
    for it in range(3):
        culled = (torch.rand(n, generator=gen) < 0.5).to(DEV)
        if it:
            culled |= was_culled   # a row seeded before stays culled, so every visible row starts finite
        rows = culled.nonzero().squeeze(1)
        tw.set_grads()
        held = []
        with torch.no_grad():
            for p in tw.p:
                st = tw.sel.state[p]
                for t in (p, st["exp_avg"], st["exp_avg_sq"], p.grad):
                    pick = torch.randint(0, 5, (len(rows), p.shape[1]), generator=gen).to(DEV)
                    t[rows] = odd[pick]
                    t[rows[0], 0] = nan_payload[0]
                held.append([bits(t)[rows].clone() for t in (p, st["exp_avg"], st["exp_avg_sq"])])
        tw.sel.step(culling_mask=culled)
        for i, p in enumerate(tw.p):
            st = tw.sel.state[p]
            for name, t, h in zip(("param", "exp_avg", "exp_avg_sq"), (p, st["exp_avg"], st["exp_avg_sq"]), held[i]):
                assert torch.equal(bits(t)[rows], h), (it, i, name)
                assert torch.isfinite(t[~culled]).all(), (it, i, name)
        assert all(s.intact() for s in tw.slabs)
        was_culled = culled
    assert int((~was_culled).sum()) > 50


def test_every_launch_path_grid_cap_second_trip_and_a_group_boundary_inside_a_stride(monkeypatch):
    n = 300_001
    tw = Twin(n, seed=3, device_rand=True)
    sizes = tuple(n * w for w in WIDTHS)
    ends, c = [], 0
    for s in sizes:
        c += (s + 3) // 4
        ends.append(c)
    assert ends[-1] > 2 * STRIDE                       # the cap bites (every thread of trip one holds two chunks), a second trip runs
    assert 0 < ends[0] < STRIDE and ends[4] < STRIDE   # group boundaries strictly inside the first stride ...
    assert ends[0] + STRIDE < ends[5]                  # ... so pairs (c, c + STRIDE) lie in two tensors: the small ones and sh
    assert sizes[0] % 4 and sizes[5] % 4               # tail chunks, in the first slot and in the last trip
    assert ends[VIEW - 1] < ends[VIEW] < STRIDE        # the misaligned view: scalar path in the first slot
    launches = spy_on_launches(monkeypatch)
    gen = torch.Generator().manual_seed(4)
    tw.set_grads()
    tw.step_and_compare((torch.rand(n, generator=gen) < 0.5).to(DEV))
    assert launches == [sizes]


def test_row_index_beyond_32_bits():
    """one [2^28 + 1000, 8] tensor: more than 2^31 elements, so the row of a chunk comes from the 64-bit division.  The
    tensors are not initialised (8.6 GB each); a handful of rows at both ends, in the middle and on both sides of
    element 2^31 are visible and compared with a dense step over just those rows, the stretches of culled rows next
    to them must keep their bits."""
    n, w = (1 << 28) + 1000, 8
    assert n * w > 2 ** 31 - 1
    gen = torch.Generator().manual_seed(5)
    p = torch.empty(n, w, device=DEV).requires_grad_(True)
    p.grad = torch.empty(n, w, device=DEV)
    m, v = torch.empty(n, w, device=DEV), torch.empty(n, w, device=DEV)
    rows = torch.tensor([0, 1, n // 2, (1 << 28) - 3, (1 << 28) + 5, n - 2, n - 1])
    small = [torch.randn(len(rows), w, generator=gen).to(DEV) for _ in range(4)]
    small[3].abs_()
    with torch.no_grad():
        for t, s in zip((p, p.grad, m, v), small):
            t[rows.to(DEV)] = s
    near = []   # up to 3000 culled rows behind and in front of every visible row
    for a, b in zip(rows[:-1].tolist(), rows[1:].tolist()):
        if b - a > 1:
            near += [slice(a + 1, min(b, a + 3001)), slice(max(a + 1, b - 3000), b)]
    held = [[bits(t[s]).clone() for s in near] for t in (p, m, v)]
    culled = torch.ones(n, dtype=torch.bool, device=DEV)
    culled[rows.to(DEV)] = False
    opt = SelectiveAdam([p], lr=0.01)
    opt.state[p] = {"step": torch.tensor(41.0), "exp_avg": m, "exp_avg_sq": v}
    q = small[0].clone().requires_grad_(True)
    q.grad = small[1].clone()
    ref = Adam([q], lr=0.01)
    ref.state[q] = {"step": torch.tensor(41.0), "exp_avg": small[2].clone(), "exp_avg_sq": small[3].clone()}
    ref.step()
    opt.step(culling_mask=culled)
    for name, t, r in (("param", p.detach(), q.detach()), ("exp_avg", m, ref.state[q]["exp_avg"]),
                       ("exp_avg_sq", v, ref.state[q]["exp_avg_sq"])):
        assert torch.equal(t[rows.to(DEV)], r), name
    for t, hs in zip((p, m, v), held):
        for s, h in zip(near, hs):
            assert torch.equal(bits(t[s]), h)
    del p, m, v, culled, opt, held
    torch.cuda.empty_cache()   # 35 GB go back to the device, not to this process's cache


def spy_on_launches(monkeypatch):
    """-> list that receives the numel tuple of every gs_adam_step_rows launch; a dense gs_adam_step of `sel` would be
    a quiet fall-back and is not booked"""
    launches, real = [], _hip.call

    def call(name, *args):
        if name == "gs_adam_step_rows":
            launches.append(tuple(args[5][i] for i in range(args[0])))
            assert tuple(args[6][i] * args[8] for i in range(args[0])) == launches[-1]   # row_width * n_rows
        return real(name, *args)

    monkeypatch.setattr(_hip, "call", call)
    return launches


@pytest.mark.parametrize("layout", ["one_group", "betas_in_the_middle"])
def test_masked_step_splits_its_launches(monkeypatch, layout):
    n = 101
    widths = tuple(1 + i for i in range(10))
    sizes = [n * w for w in widths]
    other = (0.8, 0.99)
    idle = torch.randn(n, 2, device=DEV).requires_grad_(True)   # grad None: skipped, no state
    idle_before = idle.detach().clone()
    if layout == "one_group":
        mk = lambda ts: [{"params": ts[:4] + [idle] + ts[4:], "lr": 0.004}]
        want = [tuple(sizes[:8]), tuple(sizes[8:])]
    else:
        mk = lambda ts: [{"params": ts[:3], "lr": LRS[0]}, {"params": [ts[3], idle, ts[4]], "lr": LRS[2], "betas": other},
                         {"params": ts[5:], "lr": LRS[3]}]
        want = [tuple(sizes[:3]), tuple(sizes[3:5]), tuple(sizes[5:])]
    step0 = tuple(None if i % 3 == 0 else 10 * i for i in range(10))
    tw = Twin(n, widths=widths, step0=step0, view=7, seed=23, groups=mk)
    gen = torch.Generator().manual_seed(24)
    tw.set_grads()
    launches = spy_on_launches(monkeypatch)
    tw.step_and_compare((torch.rand(n, generator=gen) < 0.5).to(DEV))
    assert launches == want
    assert torch.equal(idle, idle_before) and len(tw.sel.state[idle]) == 0


def test_state_layout_survives_the_reference_surgery_between_masked_steps():
    """test_adam_state_layout_survives_the_reference_surgery with SelectiveAdam, and the surgery itself:
    OptimizerManager.delete_gaussians / add_gaussians (optimizer_manager.py:78-172) reach into optimizer.state[param]
    and param_groups[i]["params"][0], masked steps before and after"""
    n = 500
    gen = torch.Generator().manual_seed(31)
    tw = Twin(n, widths=WIDTHS[:5], lrs=LRS[:5], step0=(None,) * 5, view=None, seed=30)
    tw.set_grads()
    tw.step_and_compare((torch.rand(n, generator=gen) < 0.4).to(DEV), "before")
    st = tw.sel.state[tw.sel.param_groups[3]["params"][0]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["exp_avg"].shape == (n, 1)
    keep = (torch.rand(n, generator=gen) < 0.7).to(DEV)
    extra = 77
    for opt, ts in ((tw.sel, tw.p), (tw.ref, tw.q)):
        for i, group in enumerate(opt.param_groups):
            old = group["params"][0]
            state = opt.state.pop(old)
            new = torch.cat((old.detach()[keep], old.detach()[:extra] * 0.5)).requires_grad_(True)
            state["exp_avg"] = torch.cat((state["exp_avg"][keep], torch.zeros_like(old[:extra])))
            state["exp_avg_sq"] = torch.cat((state["exp_avg_sq"][keep], torch.zeros_like(old[:extra])))
            group["params"][0] = new
            opt.state[new] = state
            ts[i] = new
    tw.slabs = []
    n2 = int(keep.sum()) + extra
    for it in range(2):
        tw.set_grads()
        tw.step_and_compare((torch.rand(n2, generator=gen) < 0.4).to(DEV), f"after {it}")
    assert all(float(tw.sel.state[p]["step"]) == 3 for p in tw.p)
    # a tensor the kernel does not take (fp64) goes through torch's functional Adam on its visible rows
    q = torch.zeros(5, dtype=torch.float64, device=DEV, requires_grad=True)
    q.grad = torch.ones_like(q)
    opt2 = SelectiveAdam([q], lr=0.1)
    opt2.step(culling_mask=torch.tensor([False, True, False, True, True], device=DEV))
    assert torch.allclose(q.detach(), torch.tensor([-0.1, 0, -0.1, 0, 0], dtype=torch.float64, device=DEV))
    assert float(opt2.state[q]["step"]) == 1


def test_training_iterations_with_the_frames_own_mask():
    """test_training_iterations_reduce_the_loss with SelectiveAdam.  cull_mask_padding=0: the Gaussians whose centre
    projects outside the image (about 1/6 per axis, synthetic.make_scene) are culled"""
    from gaussian_splatting_amd import fused
    from gaussian_splatting_amd.train_ops import ssim_l1_loss
    N, W, H = 4000, 192, 128
    args = dict(near_thresh=0.3, far_thresh=500.0, cull_mask_padding=0, mh_dist=3.0, use_sh_precompute=True,
                background_rgb=torch.zeros(3, device=DEV))
    g, cam, T = make_scene(N, W, H, 1, seed=11, device=DEV)
    with torch.no_grad():
        target, _, _ = fused.rasterize(g, T, cam, **args)
        gen = torch.Generator().manual_seed(3)
        g.rgb.add_(0.5 * torch.randn(g.rgb.shape, generator=gen).to(DEV))
        g.xyz.add_(0.02 * torch.randn(g.xyz.shape, generator=gen).to(DEV))
    start = {k: getattr(g, k).detach().clone() for k in NAMES}
    for k in NAMES:
        getattr(g, k).requires_grad_(True)
    opt = SelectiveAdam([{"params": getattr(g, k), "lr": lr} for k, lr in zip(NAMES, LRS)])
    never_seen = torch.ones(N, dtype=torch.bool, device=DEV)
    losses = []
    for it in range(40):
        opt.zero_grad(set_to_none=True)
        img, culled, uv = fused.rasterize(g, T, cam, **args)
        assert bool(culled.any()) and not bool(culled.all())
        loss = ssim_l1_loss(img, target, 0.2)
        loss.backward()
        opt.step(culling_mask=culled)
        never_seen &= culled
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.6 * losses[0], (losses[0], losses[-1])
    assert int(never_seen.sum()) > 0
    for k in NAMES:
        p = getattr(g, k)
        st = opt.state[p]
        assert float(st["step"]) == 40
        assert torch.equal(bits(p)[never_seen], bits(start[k])[never_seen]), k
        assert not bits(st["exp_avg"])[never_seen].any() and not bits(st["exp_avg_sq"])[never_seen].any(), k
        assert not torch.equal(p.detach()[~never_seen], start[k][~never_seen]), k
