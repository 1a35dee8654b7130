"""Render records whose float32 determinant is degenerate, made by hand (test code only).

The fp32 render record holds a = conic0 + 1/4, b = conic1 / 2, c = conic2 + 1/4, det = a c - b b (two rounded products,
one difference) and 1 / det.  The classes, exact by construction (classify() restates the record's arithmetic in
numpy float32 and the GPU test asserts them again on the kernel's own packed record):

  zero    det == 0: 1 / det = inf, the cutoff radius is inf, the quadratic form times 1 / det is never a finite positive
          number, so no pixel takes the splat and the reference leaves all its gradients at +0
  neg     det < 0: the form is indefinite, the splat contributes where form / det > 0; the reference has no guard
  noisy   det > 0 and equal to ONE ulp of a c while the exact a c - b^2 of the same fp32 a, b, c is 0.3 .. 3 times
          that: the record's determinant is rounding noise
  plain   everything else

each at a small magnitude (a, c ~ 4) and at the magnitude of an extreme needle (a, c ~ 1e8, where b is found by a
search over neighbouring floats).  Scenes are render_ref64._scene namespaces (run_module / oracle_run take them)."""
import functools

import numpy as np
import torch

from . import render_ref64 as R

F = np.float32
CLASSES = ("zero", "neg", "noisy")
A_BIG, C_BIG = 143023488.0, 138057696.0   # a needle seen at 45 degrees: a ~ c ~ |b| ~ 1.4e8


def record_abc(conic):
    """a, b, c, det of the fp32 record for conic [V, 3] (numpy float32 arithmetic, the record's operation order)"""
    k = np.asarray(conic, dtype=F)
    a, b, c = k[:, 0] + F(0.25), k[:, 1] * F(0.5), k[:, 2] + F(0.25)
    det = (a * c).astype(F) - (b * b).astype(F)
    return a, b, c, det.astype(F)


def classify(conic):
    """-> list of class names ("zero" | "neg" | "noisy" | "plain") of conic [V, 3]: tests/ref64.py's det_classes, the one
    statement of the rule"""
    from .ref64 import det_classes
    return list(det_classes(torch.as_tensor(np.asarray(conic, dtype=F))))


@functools.lru_cache(maxsize=None)
def big_conic(cls, sign=1.0):
    """(conic0, conic1, conic2) at needle magnitude of class cls: b searched among the floats next to sqrt(a c)"""
    a, c = F(A_BIG), F(C_BIG)
    for _ in range(256):   # (one step of b moves b^2 by about two ulps of a c: c is stepped too)
        b = F(np.sqrt(np.float64(a) * np.float64(c)))
        up = down = b
        for _ in range(16):
            for cand in (up, down):
                conic = (float(a), float(F(2.0) * cand) * sign, float(c))   # (+ 1/4 is below half an ulp of a, c)
                if classify([conic])[0] == cls:
                    ra, rb, rc, _ = record_abc([conic])
                    assert ra[0] == a and rc[0] == c and abs(rb[0]) == cand
                    return conic
            up, down = np.nextafter(up, F(np.inf)), np.nextafter(down, F(-np.inf))
        c = np.nextafter(c, F(np.inf))
    raise AssertionError(f"no b next to sqrt(a c) gives class {cls}")


SMALL = {"zero": (3.75, 8.0, 3.75),     # a = c = b = 4
         "neg": (3.75, 8.25, 3.75)}     # b = 4.125: det = -1.015625


def conic_of(cls, big, sign=1.0):
    if big:
        return big_conic(cls, sign)
    k = SMALL[cls]   # (no small noisy record: one ulp of a c ~ 16 is 2e-6, a determinant nobody mistakes for noise)
    return (k[0], k[1] * sign, k[2])


def _assemble(name, W, H, rows, lists, bg, seed):
    """rows: list of (u, v, conic3, opacity, class or None)"""
    uv = torch.tensor([[r[0], r[1]] for r in rows], dtype=torch.float64)
    conic = torch.tensor([list(r[2]) for r in rows], dtype=torch.float64)
    opacity = torch.tensor([r[3] for r in rows], dtype=torch.float64)
    sorted_g, ranges = lists
    sc = R._scene(name, W, H, uv, conic, opacity, sorted_g, ranges, bg, seed)
    sc.want = [r[4] or "plain" for r in rows]
    sc.got = classify(sc.conic.numpy())
    sc.rows = {cls: torch.tensor([i for i, w in enumerate(sc.want) if w == cls], dtype=torch.long)
               for cls in CLASSES + ("plain",)}
    sc.z = (1.0 + 0.05 * torch.arange(sc.V, dtype=torch.float64)).float()   # the list order is the depth order
    return sc


@functools.lru_cache(maxsize=None)
def scene_a():
    """48 x 32, six tiles, 40 splats in index (= depth) order, every tile's list names all of them (a list may name a
    splat that does not reach its tile: the cutoff radius and the alpha test decide).  Twelve degenerate records
    between 28 ordinary ones: centred on the screen, on the corner four tiles share, and off the screen within the
    cull padding."""
    gen = torch.Generator().manual_seed(31)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    centre, corner, off_l, off_b = (24.3, 15.6), (16.0, 16.0), (-40.0, 10.0), (60.0, 50.0)
    special = {2: ("zero", False, centre, 1.0), 5: ("zero", True, centre, 1.0), 8: ("neg", False, centre, 1.0),
               11: ("noisy", True, centre, -1.0), 14: ("zero", False, corner, -1.0), 17: ("neg", True, corner, 1.0),
               20: ("noisy", True, corner, 1.0), 23: ("neg", False, corner, -1.0), 26: ("zero", True, off_l, -1.0),
               29: ("neg", True, off_b, -1.0), 32: ("noisy", True, off_l, 1.0), 35: ("zero", False, off_b, 1.0)}
    rows = []
    for i in range(40):
        if i in special:
            cls, big, (u, v), sign = special[i]
            rows.append((u, v, conic_of(cls, big, sign), 0.3 + 0.4 * float(rnd(1)), cls))
        else:
            sig = 1.0 + 2.5 * rnd(2)
            rho = 1.6 * (float(rnd(1)) - 0.5)
            conic = (float(sig[0] ** 2), float(2 * rho * sig[0] * sig[1]), float(sig[1] ** 2))
            rows.append((float(48 * rnd(1)), float(32 * rnd(1)), conic, 0.05 + 0.6 * float(rnd(1)), None))
    lists = (torch.arange(40).repeat(6), torch.arange(7) * 40)
    return _assemble("degenerate_48x32", 48, 32, rows, lists, 0.5, 1031)


B_CHUNK = 64                      # GS_BWD_CHUNK: entries the backward stages at a time
B_STACK = (20, 21, 22)            # three opaque splats in the corner: the pixels under them stop there
B_SPECIAL = {10: ("zero", False), 40: ("zero", True), 45: ("neg", False), 50: ("noisy", True),   # chunk 0: others hit
             100: ("zero", False), 101: ("zero", True),                                           # chunk 1: nobody hits
             140: ("zero", False), 141: ("neg", True)}                                            # chunk 2


@functools.lru_cache(maxsize=None)
def scene_b():
    """one 16 x 16 tile, 150 entries in index order = three chunks of the backward.  Chunk 0 and chunk 2 hold faint
    ordinary splats that every pixel takes; chunk 1 holds only splats below the alpha threshold (opacity 0.003) and two
    det == 0 records: a chunk that is staged and that nobody hits.  Entries 20 .. 22 are opaque and small: the pixels in
    their corner saturate there, in front of entry 40 and behind entry 10."""
    gen = torch.Generator().manual_seed(32)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    rows = []
    for i in range(150):
        u, v = float(16 * rnd(1)), float(16 * rnd(1))
        conic = (20.0 + 30.0 * float(rnd(1)), 4.0 * (float(rnd(1)) - 0.5), 20.0 + 30.0 * float(rnd(1)))
        if i in B_SPECIAL:
            cls, big = B_SPECIAL[i]
            rows.append((2.0 + 12.0 * float(rnd(1)), 2.0 + 12.0 * float(rnd(1)), conic_of(cls, big), 0.4, cls))
        elif i in B_STACK:
            rows.append((3.3, 3.4, (30.0, 0.0, 30.0), 0.995, None))   # (off the pixel grid: m = 0 is not taken)
        elif B_CHUNK <= i < 2 * B_CHUNK:
            rows.append((u, v, conic, 0.003, None))
        else:
            rows.append((u, v, conic, 0.002 + 0.018 * float(rnd(1)), None))
    lists = (torch.arange(150), torch.tensor([0, 150]))
    return _assemble("degenerate_one_tile", 16, 16, rows, lists, 0.5, 1032)


SCENES = {"A": scene_a, "B": scene_b}


def without_rows(sc, drop):
    """the scene with the list entries of Gaussians `drop` taken out of every tile's list (the arrays stay)"""
    from types import SimpleNamespace
    keep_mask = torch.ones(sc.V, dtype=torch.bool)
    keep_mask[drop] = False
    sorted_g, ranges = [], [0]
    for t in range(sc.ranges.numel() - 1):
        seg = sc.sorted_g[int(sc.ranges[t]):int(sc.ranges[t + 1])].long()
        seg = seg[keep_mask[seg]]
        sorted_g.append(seg)
        ranges.append(ranges[-1] + seg.numel())
    out = SimpleNamespace(**vars(sc))
    out.sorted_g = torch.cat(sorted_g).int().contiguous()
    out.ranges = torch.tensor(ranges, dtype=torch.int32)
    return out


def oracle_render(sc, n_sh=1, exact=True):
    """the CPU oracle's fp32 render forward, backward and backward abs sums of scene sc -> dict keyed as
    tests/test_gpu_scale.py's check_band_backward reads it (image, nsp, fw, g_*, a_*)"""
    from oracle import gs_oracle
    gs_oracle.set_modes(0, 0)
    gs_oracle.set_sh_band1_mode(0)
    H, W, V = sc.H, sc.W, sc.V
    colour = R.scene_coeff(sc, n_sh)
    rays = sc.rays if n_sh > 1 else torch.zeros(1, 1, 1)
    img, nsp, fw = torch.zeros(H, W, 3), torch.zeros(H, W, dtype=torch.int32), torch.zeros(H, W)
    args = (sc.uv, sc.opacity, colour, sc.conic, rays, sc.ranges, sc.sorted_g, sc.bg)
    gs_oracle.render_tiles_cuda(*args, nsp, fw, img)
    shapes = (tuple(colour.shape), (V, 1), (V, 2), (V, 3))
    g = [torch.zeros(*sh) for sh in shapes]
    a = [torch.zeros(*sh) for sh in shapes]
    try:
        gs_oracle.set_backward_exact(int(exact))
        gs_oracle.render_tiles_backward_cuda(*args, nsp, fw, sc.grad_image, *g)
        gs_oracle.render_tiles_backward_abs(*args, nsp, fw, sc.grad_image, *a)
    finally:
        gs_oracle.set_backward_exact(0)
    return dict(image=img, nsp=nsp, fw=fw, g_rgb=g[0], g_opa=g[1], g_uv=g[2], g_conic=g[3], a_rgb=a[0], a_opa=a[1],
                a_uv=a[2], a_conic=a[3])


GRADS = ("g_rgb", "g_opa", "g_uv", "g_conic")


def check_degenerate_gradients(sc, grads):
    """criterion (c) without the oracle: grads (dict of GRADS [V, ...]) finite everywhere, the det == 0 rows exactly +0"""
    zero = sc.rows["zero"]
    for k in GRADS:
        g = grads[k].reshape(sc.V, -1)
        assert bool(torch.isfinite(g).all()), (k, torch.nonzero(~torch.isfinite(g).all(dim=1)).flatten().tolist())
        assert not g[zero].any(), (k, "det == 0 rows", g[zero])
        assert not torch.signbit(g[zero]).any(), (k, "det == 0 rows hold -0")


@functools.lru_cache(maxsize=None)
def scene_fp64():
    """scene A for the float64 kernels, which take the conic without the dilation: det == 0 is (4, 8, 4), det < 0 is
    (4, 8.25, 4), both exact in either precision; the needle-magnitude slots hold an ordinary needle (correlation 0.995).
    float64 has no one-ulp class to speak of: a c - b^2 of these values is exact."""
    a = scene_a()
    conic = a.conic.double().clone()
    want = []
    for i, w in enumerate(a.want):
        if w == "plain":
            want.append("plain")
        elif float(conic[i, 0]) > 1e6 or w == "noisy":
            conic[i] = torch.tensor([60.0, 2 * 0.995 * (60.0 * 0.4) ** 0.5 * (1 if float(conic[i, 1]) > 0 else -1), 0.4])
            want.append("plain")
        else:
            sign = 1.0 if float(conic[i, 1]) > 0 else -1.0
            conic[i] = torch.tensor([4.0, (8.0 if w == "zero" else 8.25) * sign, 4.0])
            want.append(w)
    from types import SimpleNamespace
    sc = SimpleNamespace(**vars(a))
    sc.name, sc.conic, sc.want = "degenerate_48x32_fp64", conic.float().contiguous(), want
    det = conic[:, 0] * conic[:, 2] - 0.25 * conic[:, 1] ** 2
    sc.rows = {c: torch.tensor([i for i, w in enumerate(want) if w == c], dtype=torch.long) for c in CLASSES + ("plain",)}
    assert bool((det[sc.rows["zero"]] == 0).all()) and bool((det[sc.rows["neg"]] < 0).all()) and bool((det[sc.rows["plain"]] > 0).all())
    return sc
