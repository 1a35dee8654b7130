"""The depth cut's contract (csrc/binning.hip "depth cut", include/gsplat_hip.h) restated in plain CPU code on top of
COMPLETE tile lists -- the oracle's (oracle.gs_oracle.get_sorted_gaussian_list), never the HIP path's.

Every quantity is an integer and every comparison with the device is exact.  The bucket boundaries are an INPUT of the
restatement (they are sample quantiles: any ascending set is a valid one, check_bounds states what is promised of
them); everything behind them is determined:

  bucket of a Gaussian   the first of the first 1023 boundaries that is >= its depth's sortable bits, else 1023
  b*(t)                  the last non-empty bucket of tile t at which the tile's cumulative count is <= kcut;
                         -1 if already its first non-empty bucket holds more, and -1 for an empty tile
  kept count n'(t)       the cumulative count there (0 for b* = -1); all entries whenever the tile has <= kcut
  kept list              the first n'(t) entries of the complete list (buckets are depth intervals and equal depths
                         share a bucket, so a union of leading buckets is a depth prefix)
  flags                  a truncated tile that reaches the end of its kept list with an unsaturated pixel is repaired
                         from its complete list (flag_bounds)
"""
from types import SimpleNamespace

import torch

N_BUCKETS = 1024


def sortable(z):
    """the sortable depth bits of float32 depths (csrc/tile_math.h): a < b as floats iff sortable(a) < sortable(b) as
    unsigned integers; -> int64 in [0, 2^32)"""
    u = z.contiguous().view(torch.int32).long() & 0xffffffff
    return torch.where(u >= 0x80000000, (~u) & 0xffffffff, u | 0x80000000)


def _unsigned(x):
    return x.long() & 0xffffffff


def check_bounds(bounds, near, far, any_visible):
    """the documented properties of the device's bucket boundaries uint32[1024] (inclusive upper bounds in sortable
    bits): ascending, the last one all ones and, when anything is visible, the others inside [near, far]"""
    b = _unsigned(bounds)
    assert b.numel() == N_BUCKETS
    assert bool((b[1:] >= b[:-1]).all()), "bucket boundaries must ascend"
    assert int(b[-1]) == 0xffffffff
    if any_visible:
        lo, hi = (int(x) for x in sortable(torch.tensor([near, far], dtype=torch.float32)))
        assert lo <= int(b[0]) and int(b[N_BUCKETS - 2]) <= hi, (lo, int(b[0]), int(b[N_BUCKETS - 2]), hi)


def bucket_of(keys, bounds):
    """bucket of every key (sortable bits, int64): the first of the first 1023 bounds that is >= the key, else 1023"""
    b = _unsigned(bounds)[:N_BUCKETS - 1].contiguous()
    return torch.searchsorted(b, keys.long().contiguous(), right=False)


def cut_reference(ranges, sorted_g, keys, bounds, kcut=1024, rows=None, ntx=None):
    """ranges [T+1], sorted_g [S]: the complete lists; keys [V]: sortable(z) of every visible Gaussian; bounds: the
    device's boundaries.  rows = (r0, r1) with ntx tiles per row: only tile rows [r0, r1) are binned, every other tile
    is empty (its bstar is meaningless: -1 here).
    -> totals, bstar, kept, kept_ranges, full_ranges, kept_sorted (the kept lists one after the other), populations
    (entries of each bucket over all visible Gaussians), deepest (max bstar), in_band [T] bool"""
    ranges, sorted_g = ranges.long(), sorted_g.long()
    T = ranges.numel() - 1
    in_band = torch.ones(T, dtype=torch.bool)
    if rows is not None:
        tile_row = torch.arange(T) // ntx
        in_band = (tile_row >= rows[0]) & (tile_row < rows[1])
    bucket = bucket_of(keys, bounds)
    totals = torch.zeros(T, dtype=torch.long)
    kept = torch.zeros(T, dtype=torch.long)
    bstar = torch.full((T,), -1, dtype=torch.long)
    kept_lists = []
    for t in range(T):
        if not in_band[t]:
            continue
        lst = sorted_g[ranges[t]:ranges[t + 1]]
        totals[t] = lst.numel()
        cum = torch.cumsum(torch.bincount(bucket[lst], minlength=N_BUCKETS), 0)
        per = torch.diff(cum, prepend=torch.zeros(1, dtype=torch.long))
        ok = torch.nonzero((per > 0) & (cum <= kcut)).flatten()
        if ok.numel():
            bstar[t] = int(ok[-1])
            kept[t] = int(cum[ok[-1]])
        kept_lists.append(lst[:int(kept[t])])
    zero = torch.zeros(1, dtype=torch.long)
    return SimpleNamespace(
        totals=totals, bstar=bstar, kept=kept, in_band=in_band,
        kept_ranges=torch.cat([zero, torch.cumsum(kept, 0)]), full_ranges=torch.cat([zero, torch.cumsum(totals, 0)]),
        kept_sorted=torch.cat(kept_lists) if kept_lists else torch.zeros(0, dtype=torch.long),
        populations=torch.bincount(bucket, minlength=N_BUCKETS), deepest=int(bstar.max()) if T else -1)


def flag_bounds(kept, totals, nsp_full, W, H, tile=16):
    """The flag rule as two sets of tiles (bool [T] each).  nsp_full [H, W]: num_splats_per_pixel of the render of the
    COMPLETE lists.  must: truncated tiles (kept < totals) with a pixel that composites deeper than the kept prefix
    (num_splats > kept); may: must plus the truncated tiles whose deepest pixel stops exactly at the end of the prefix
    (max num_splats == kept: such a pixel may or may not count as saturated there).  A correct frame has
    must <= flags <= may."""
    ntx, nty = (W + tile - 1) // tile, (H + tile - 1) // tile
    pad = torch.zeros(nty * tile, ntx * tile, dtype=torch.long)
    pad[:H, :W] = nsp_full.long()
    deepest = pad.view(nty, tile, ntx, tile).amax(dim=(1, 3)).reshape(-1)
    truncated = kept.long() < totals.long()
    must = truncated & (deepest > kept.long())
    may = must | (truncated & (deepest == kept.long()))
    return must, may
