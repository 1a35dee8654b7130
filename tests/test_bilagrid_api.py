"""The bilateral-grid entry points exist where their callers look for them (no GPU needed): the built library exports
the five symbols at ABI 23 and _hip types them from the header, the C entries refuse bad arguments before any device
call, the backward's workspace follows the integer cell partition, bilagrid.slice / total_variation_loss refuse by name
what they do not serve, and BilateralGrid starts as the identity."""
import ctypes

import pytest
import torch

from gaussian_splatting_amd import _hip, bilagrid

SYMBOLS = ("gs_bilagrid_workspace_bytes", "gs_bilagrid_slice", "gs_bilagrid_slice_backward",
           "gs_bilagrid_tv_workspace_bytes", "gs_bilagrid_tv")


def test_library_exports_the_entry_points_at_abi_23():
    raw = ctypes.CDLL(_hip.LIB_PATH)
    lib = _hip.lib()
    assert lib.gs_abi_version() >= 23
    P, I, Z, Q = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int64
    want = {"gs_bilagrid_workspace_bytes": (Z, [I] * 5),
            "gs_bilagrid_slice": (I, [P, P] + [I] * 5 + [P, P]),
            "gs_bilagrid_slice_backward": (I, [P] * 3 + [I] * 5 + [P] * 4),
            "gs_bilagrid_tv_workspace_bytes": (Z, [Q, I, I, I]),
            "gs_bilagrid_tv": (I, [P, Q, I, I, I] + [P] * 4)}
    for n in SYMBOLS:
        assert hasattr(raw, n), n
        assert n in _hip.EXPORTS
        fn = getattr(lib, n)
        assert (fn.restype, list(fn.argtypes)) == (want[n][0], want[n][1]), n


def test_c_entries_refuse_bad_arguments_before_any_device_call():
    lib = _hip.lib()
    einval = _hip.GS_EINVAL
    one = ctypes.c_void_p(16)   # never dereferenced: the checks come first
    assert lib.gs_bilagrid_slice(None, one, 4, 4, 1, 1, 1, one, None) == einval
    assert b"bilagrid_slice" in lib.gs_last_error()
    assert lib.gs_bilagrid_slice(one, one, 0, 4, 1, 1, 1, one, None) == einval
    assert lib.gs_bilagrid_slice(one, one, 4, 4, 1, 0, 1, one, None) == einval
    assert lib.gs_bilagrid_slice_backward(one, one, None, 4, 4, 1, 1, 1, one, one, one, None) == einval
    assert lib.gs_bilagrid_slice_backward(one, one, one, 4, 4, 0, 1, 1, one, one, one, None) == einval
    assert lib.gs_bilagrid_slice_backward(one, one, one, 4, 4, 1, 1, 1, None, one, one, None) == einval   # no workspace
    assert lib.gs_bilagrid_tv(one, 0, 1, 1, 1, one, one, None, None) == einval
    assert lib.gs_bilagrid_tv(one, 1, 1, 1, 1, one, None, None, None) == einval
    assert b"bilagrid_tv" in lib.gs_last_error()


@pytest.mark.parametrize("H,W,L,Hg,Wg", [(840, 1297, 8, 16, 16), (45, 70, 4, 5, 3), (500, 11, 8, 16, 16),
                                         (13, 701, 8, 16, 16), (1, 1, 1, 1, 1), (7, 9, 3, 1, 16), (1080, 1920, 8, 2, 1)])
def test_workspace_follows_the_integer_cell_partition(H, W, L, Hg, Wg):
    """one 256-lane workgroup per chunk of 1024 pixels of one xy cell, 4 L 12 fp32 partials each; the cell of a pixel is
    (2 p + 1)(n - 1) div (2 N), here by brute force"""
    def largest_cell(N, n):
        if n < 2:
            return N
        cells = [min(((2 * p + 1) * (n - 1)) // (2 * N), n - 2) for p in range(N)]
        return max(cells.count(c) for c in range(n - 1))

    chunks = max(-(-largest_cell(W, Wg) * largest_cell(H, Hg) // 1024), 1)
    want = max(Wg - 1, 1) * max(Hg - 1, 1) * chunks * L * 48 * 4
    assert _hip.lib().gs_bilagrid_workspace_bytes(H, W, L, Hg, Wg) == want
    assert _hip.lib().gs_bilagrid_workspace_bytes(0, W, L, Hg, Wg) == 0


def test_tv_workspace_is_one_double_per_workgroup():
    """256 lanes of 16 elements each"""
    assert _hip.lib().gs_bilagrid_tv_workspace_bytes(3, 8, 16, 16) == -(-3 * 12 * 8 * 16 * 16 // 4096) * 8
    assert _hip.lib().gs_bilagrid_tv_workspace_bytes(1, 1, 1, 1) == 8
    assert _hip.lib().gs_bilagrid_tv_workspace_bytes(0, 1, 1, 1) == 0


def test_slice_refuses_by_name_before_any_device_call():
    grid, image = torch.zeros(12, 2, 3, 3), torch.zeros(5, 6, 3)
    with pytest.raises(RuntimeError, match="must be on one GPU device"):
        bilagrid.slice(grid, image)
    with pytest.raises(RuntimeError, match="takes tensors"):
        bilagrid.slice(grid, None)
    with pytest.raises(RuntimeError, match="float32 device tensor"):
        bilagrid.total_variation_loss(grid)
    with pytest.raises(RuntimeError, match="must be on one GPU device"):
        bilagrid.BilateralGrid(2, 3, 3, 2)(image, 0)
    # dtype and shape are judged before the device
    for bad_grid, bad_image, text in ((grid.double(), image, "float32"), (grid, image.half(), "float32"),
                                      (torch.zeros(11, 2, 3, 3), image, r"grid must be \[12, L, Hg, Wg\]"),
                                      (torch.zeros(12, 3, 3), image, r"grid must be \[12, L, Hg, Wg\]"),
                                      (torch.zeros(12, 0, 3, 3), image, r"grid must be \[12, L, Hg, Wg\]"),
                                      (grid, torch.zeros(5, 6, 4), r"image must be \[H, W, 3\]"),
                                      (grid, torch.zeros(3, 5, 6), r"image must be \[H, W, 3\]"),
                                      (grid, torch.zeros(5, 6), r"image must be \[H, W, 3\]")):
        with pytest.raises(RuntimeError, match=text):
            bilagrid.slice(bad_grid, bad_image)


def test_bilateral_grid_starts_as_the_identity():
    bil = bilagrid.BilateralGrid(3)
    assert isinstance(bil.grids, torch.nn.Parameter) and bil.grids.requires_grad
    assert bil.grids.shape == (3, 12, 8, 16, 16) and bil.grids.dtype == torch.float32
    bil = bilagrid.BilateralGrid(2, grid_x=5, grid_y=4, grid_l=3)
    assert bil.grids.shape == (2, 12, 3, 4, 5)
    A = bil.grids.detach().permute(0, 2, 3, 4, 1).reshape(-1, 3, 4)
    assert torch.equal(A, torch.eye(3, 4).expand_as(A))
    assert [n for n, _ in bil.named_parameters()] == ["grids"]
