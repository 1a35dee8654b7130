"""tests/cut_ref.py (the depth cut's contract restated on complete lists) against answers worked out by hand."""
import pytest
import torch

from .cut_ref import bucket_of, check_bounds, cut_reference, flag_bounds, sortable


def u32(x):
    """int64 values in [0, 2^32) as the int32 bits the device's uint32 arrays are read back as"""
    return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)


# boundaries 10, 20, ..., 10230 and all ones: a key 10 b + 5 lies in bucket b, the key 10 (b + 1) still does
BOUNDS = u32(torch.cat([10 * torch.arange(1, 1024), torch.tensor([0xffffffff])]))


def lists(*tiles):
    """tiles: per tile, the bucket of every entry in list order (each entry its own Gaussian, indices descending so
    that nothing can come out right by position) -> ranges, sorted_g, keys"""
    n = sum(len(t) for t in tiles)
    ids = torch.arange(n - 1, -1, -1)
    keys = torch.zeros(n, dtype=torch.long)
    ranges, at = [0], 0
    for t in tiles:
        keys[ids[at:at + len(t)]] = 10 * torch.tensor(t, dtype=torch.long) + 5
        at += len(t)
        ranges.append(at)
    return torch.tensor(ranges, dtype=torch.int32), ids.to(torch.int32), keys


def test_sortable_orders_like_the_floats():
    z = torch.tensor([-3.0, -0.0, 0.0, 1e-40, 0.3, 6.0, 6.0000005, 500.0, float("inf")])
    s = sortable(z)
    assert bool((s[1:] > s[:-1]).all()) and int(s.min()) >= 0 and int(s.max()) < 2 ** 32
    assert int(sortable(torch.tensor([6.0]))[0]) == 0x40c00000 | 0x80000000


def test_bucket_of_takes_the_first_bound_not_below_the_key():
    keys = torch.tensor([0, 10, 11, 20, 10225, 10230, 10231, 0xfffffffe, 0xffffffff])
    assert bucket_of(keys, BOUNDS).tolist() == [0, 0, 1, 1, 1022, 1022, 1023, 1023, 1023]
    # the bounds arrive as the int32 bits of unsigned values
    hi = u32(torch.tensor([0x80000000, 0xc0000000] + [0xffffffff] * 1022))
    assert bucket_of(torch.tensor([5, 0x80000000, 0x80000001, 0xc0000001]), hi).tolist() == [0, 0, 1, 2]


def test_check_bounds_states_the_documented_properties():
    lo, hi = (int(x) for x in sortable(torch.tensor([0.3, 500.0])))
    good = torch.cat([torch.linspace(lo, hi, 1023, dtype=torch.float64).long(), torch.tensor([0xffffffff])])
    check_bounds(u32(good), 0.3, 500.0, True)
    check_bounds(torch.full((1024,), -1, dtype=torch.int32), 0.3, 500.0, False)   # nothing visible: all ones
    for bad in (good.flip(0), torch.cat([good[:-1], good[-2:-1]]), torch.cat([good[:1] - 1, good[1:]])):
        with pytest.raises(AssertionError):
            check_bounds(u32(bad), 0.3, 500.0, True)


def test_a_tile_of_1024_entries_is_kept_whole():
    r, s, k = lists([0] * 500 + [7] * 524)
    c = cut_reference(r, s, k, BOUNDS)
    assert c.totals.tolist() == [1024] and c.kept.tolist() == [1024] and c.bstar.tolist() == [7]
    assert torch.equal(c.kept_sorted, s.long()) and c.deepest == 7


def test_1025_entries_in_two_buckets_keep_the_first_bucket():
    r, s, k = lists([3] * 1000 + [4] * 25)
    c = cut_reference(r, s, k, BOUNDS)
    assert c.totals.tolist() == [1025] and c.kept.tolist() == [1000] and c.bstar.tolist() == [3]
    assert torch.equal(c.kept_sorted, s.long()[:1000])
    assert c.kept_ranges.tolist() == [0, 1000] and c.full_ranges.tolist() == [0, 1025]


def test_cumulative_count_of_exactly_1024_at_a_boundary_is_kept():
    r, s, k = lists([0] * 1000 + [5] * 24 + [6] * 3, [0] * 1000 + [5] * 24)
    c = cut_reference(r, s, k, BOUNDS)
    assert c.totals.tolist() == [1027, 1024] and c.kept.tolist() == [1024, 1024] and c.bstar.tolist() == [5, 5]
    assert bool(c.kept[0] < c.totals[0]) and bool(c.kept[1] == c.totals[1])
    # ... and with a smaller limit the same lists are cut at the boundary below it
    c = cut_reference(r, s, k, BOUNDS, kcut=1023)
    assert c.kept.tolist() == [1000, 1000] and c.bstar.tolist() == [0, 0]


def test_first_non_empty_bucket_above_the_limit_keeps_nothing():
    r, s, k = lists([9] * 1025 + [11] * 4, [2] * 3)
    c = cut_reference(r, s, k, BOUNDS)
    assert c.totals.tolist() == [1029, 3] and c.kept.tolist() == [0, 3] and c.bstar.tolist() == [-1, 2]
    assert c.kept_ranges.tolist() == [0, 0, 3] and torch.equal(c.kept_sorted, s.long()[1029:])
    assert c.deepest == 2


def test_bstar_is_a_non_empty_bucket():
    r, s, k = lists([2] * 10 + [40] * 1000 + [900] * 100)
    c = cut_reference(r, s, k, BOUNDS)
    assert c.kept.tolist() == [1010] and c.bstar.tolist() == [40]   # not 899, the last bucket with 1010 below it


def test_equal_keys_land_in_one_bucket():
    ranges = torch.tensor([0, 1030], dtype=torch.int32)
    keys = torch.full((1030,), 77, dtype=torch.long)
    keys[:5] = 12
    c = cut_reference(ranges, torch.arange(1030, dtype=torch.int32), keys, BOUNDS)
    assert c.kept.tolist() == [5] and c.bstar.tolist() == [1]       # 1025 equal keys cannot be split
    assert c.populations[1] == 5 and c.populations[7] == 1025 and int(c.populations.sum()) == 1030


def test_an_empty_tile():
    r, s, k = lists([], [1] * 4, [])
    c = cut_reference(r, s, k, BOUNDS)
    assert c.totals.tolist() == [0, 4, 0] and c.kept.tolist() == [0, 4, 0] and c.bstar.tolist() == [-1, 1, -1]
    assert c.kept_ranges.tolist() == [0, 0, 4, 4] and c.full_ranges.tolist() == [0, 0, 4, 4]
    none = cut_reference(torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.long),
                         BOUNDS)
    assert none.deepest == -1 and int(none.populations.sum()) == 0 and none.kept_sorted.numel() == 0


def test_a_gaussian_shared_by_two_tiles_counts_in_both_and_once_in_its_bucket():
    ranges = torch.tensor([0, 2, 4], dtype=torch.int32)
    sorted_g = torch.tensor([0, 1, 1, 2], dtype=torch.int32)
    c = cut_reference(ranges, sorted_g, torch.tensor([5, 15, 25]), BOUNDS)
    assert c.totals.tolist() == [2, 2] and c.bstar.tolist() == [1, 2] and c.populations[:3].tolist() == [1, 1, 1]


def test_a_row_band_empties_the_other_tiles():
    # 2 x 3 tiles, rows [1, 2): tiles 2 and 3
    r, s, k = lists([0] * 3, [1] * 2000, [2] * 1000 + [3] * 30, [4] * 5, [5] * 7, [6] * 1)
    c = cut_reference(r, s, k, BOUNDS, rows=(1, 2), ntx=2)
    assert c.in_band.tolist() == [False, False, True, True, False, False]
    assert c.totals.tolist() == [0, 0, 1030, 5, 0, 0] and c.kept.tolist() == [0, 0, 1000, 5, 0, 0]
    assert c.bstar[2:4].tolist() == [2, 4] and c.deepest == 4
    assert c.full_ranges.tolist() == [0, 0, 0, 1030, 1035, 1035, 1035]
    assert c.kept_ranges.tolist() == [0, 0, 0, 1000, 1005, 1005, 1005]
    assert torch.equal(c.kept_sorted, torch.cat([s.long()[2003:3003], s.long()[3033:3038]]))
    assert int(c.populations.sum()) == s.numel()   # the buckets hold every visible Gaussian, binned or not


def test_flag_bounds_on_three_tiles():
    """48 x 16 image: tile 0 truncated with a pixel beyond its prefix (must), tile 1 truncated with its deepest pixel
    exactly at the end of the prefix (may only), tile 2 whole and deep (never)"""
    kept, totals = torch.tensor([1000, 900, 700]), torch.tensor([1500, 1200, 700])
    nsp = torch.zeros(16, 48, dtype=torch.int32)
    nsp[:, 0:16], nsp[:, 16:32], nsp[:, 32:48] = 400, 899, 700
    nsp[3, 5], nsp[15, 31] = 1001, 900
    must, may = flag_bounds(kept, totals, nsp, 48, 16)
    assert must.tolist() == [True, False, False] and may.tolist() == [True, True, False]
    # an image that ends inside the last tile: the pixels beyond it do not exist
    must, may = flag_bounds(kept, totals, nsp[:10, :40], 40, 10)
    assert must.tolist() == [True, False, False] and may.tolist() == [True, False, False]
