"""The TSDF fusion and mesh extraction exist where their callers look for them (no GPU needed): the built library
exports the four symbols at ABI 24 and _hip types them from the header, the C entries refuse bad arguments before any
device call, mesh.TSDFVolume / integrate / integrate_views / extract_mesh / integrate_frame refuse by name what they do
not serve, and a save_ply file parses back to the arrays that went in."""
import ctypes
import math
import struct
import types

import numpy as np
import pytest
import torch

from gaussian_splatting_amd import _hip, mesh

SYMBOLS = ("gs_tsdf_integrate", "gs_tsdf_extract_workspace_bytes", "gs_tsdf_extract_count", "gs_tsdf_extract_emit")


def test_library_exports_the_entry_points_at_abi_24():
    raw = ctypes.CDLL(_hip.LIB_PATH)
    lib = _hip.lib()
    assert lib.gs_abi_version() >= 24
    P, I, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    want = {"gs_tsdf_integrate": (I, [P] * 4 + [I] * 4 + [F] * 8 + [I] * 3 + [P] * 4),
            "gs_tsdf_extract_workspace_bytes": (Z, [I] * 3),
            "gs_tsdf_extract_count": (I, [P, P, I, I, I, F, F] + [P] * 5),
            "gs_tsdf_extract_emit": (I, [P] * 6 + [I] * 3 + [F] * 5 + [P] * 4)}
    for n in SYMBOLS:
        assert hasattr(raw, n), n
        assert n in _hip.EXPORTS
        fn = getattr(lib, n)
        assert (fn.restype, list(fn.argtypes)) == (want[n][0], want[n][1]), n


def _integrate_args(**over):
    one = ctypes.c_void_p(16)   # never dereferenced: the checks come first
    a = dict(depth=one, image=one, cams=one, K=one, C=1, W=4, H=4, mode=0, near=0.2, trunc=0.2, max_w=64.0, dmax=math.inf,
             ox=0.0, oy=0.0, oz=0.0, voxel=0.05, nx=4, ny=4, nz=4, tsdf=one, weight=one, color=one, stream=None)
    a.update(over)
    return tuple(a.values())


def test_c_entries_refuse_bad_arguments_before_any_device_call():
    lib = _hip.lib()
    einval, ok = _hip.GS_EINVAL, _hip.GS_OK
    one = ctypes.c_void_p(16)
    nan = float("nan")
    for bad in (dict(image=None), dict(color=None), dict(mode=1), dict(mode=3), dict(C=-1), dict(W=-1), dict(nx=-1),
                dict(ny=262141), dict(nz=65536), dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=nan), dict(trunc=math.inf),
                dict(max_w=0.0), dict(max_w=nan), dict(near=nan), dict(dmax=nan), dict(voxel=nan), dict(ox=nan),
                dict(depth=None), dict(cams=None), dict(K=None), dict(tsdf=None), dict(weight=None)):
        assert lib.gs_tsdf_integrate(*_integrate_args(**bad)) == einval, bad
        assert b"tsdf_integrate" in lib.gs_last_error()
    assert lib.gs_tsdf_integrate(*_integrate_args(image=None)) == einval
    assert b"image and color go together" in lib.gs_last_error()
    # nothing to do: GS_OK without a launch, whatever the pointers
    for empty in (dict(C=0), dict(nx=0), dict(ny=0), dict(nz=0), dict(W=0), dict(H=0)):
        assert lib.gs_tsdf_integrate(*_integrate_args(depth=None, tsdf=None, **empty)) == ok, empty

    assert lib.gs_tsdf_extract_workspace_bytes(19, 17, 13) == 19 * 17 * 13
    assert lib.gs_tsdf_extract_workspace_bytes(0, 17, 13) == 0 and lib.gs_tsdf_extract_workspace_bytes(4, -1, 4) == 0
    count = lambda **o: lib.gs_tsdf_extract_count(*{**dict(tsdf=one, weight=one, nx=4, ny=4, nz=4, level=0.0, min_w=1.0,
                                                            ws=one, mask=one, vc=one, fc=one, stream=None), **o}.values())
    for bad in (dict(nx=-1), dict(nz=65536), dict(min_w=0.0), dict(min_w=nan), dict(level=nan), dict(tsdf=None),
                dict(weight=None), dict(ws=None), dict(mask=None), dict(vc=None), dict(fc=None)):
        assert count(**bad) == einval, bad
        assert b"tsdf_extract_count" in lib.gs_last_error()
    assert count(nx=0, tsdf=None) == ok
    emit = lambda **o: lib.gs_tsdf_extract_emit(*{**dict(tsdf=one, color=one, mask=one, vo=one, fo=one, fc=one, nx=4, ny=4,
                                                         nz=4, level=0.0, ox=0.0, oy=0.0, oz=0.0, voxel=1.0, v=one, c=one,
                                                         f=one, stream=None), **o}.values())
    for bad in (dict(ny=-1), dict(color=None), dict(c=None), dict(level=nan), dict(voxel=nan), dict(tsdf=None),
                dict(mask=None), dict(vo=None), dict(fo=None), dict(fc=None), dict(v=None), dict(f=None)):
        assert emit(**bad) == einval, bad
        assert b"tsdf_extract_emit" in lib.gs_last_error()
    assert emit(nz=0, tsdf=None) == ok


def test_volume_starts_fresh_and_resets():
    vol = mesh.TSDFVolume((0.5, -1, 2), 0.25, (5, 4, 3))
    assert vol.tsdf.shape == (3, 4, 5) and vol.weight.shape == (3, 4, 5) and vol.color.shape == (3, 4, 5, 3)
    assert all(t.dtype == torch.float32 for t in (vol.tsdf, vol.weight, vol.color))
    assert bool((vol.tsdf == 1).all()) and not vol.weight.any() and not vol.color.any()
    assert vol.sdf_trunc == 1.0 and vol.max_weight == 64.0 and vol.dims == (5, 4, 3) and vol.origin == (0.5, -1.0, 2.0)
    assert mesh.TSDFVolume((0, 0, 0), 0.1, (2, 2, 2), sdf_trunc=0.3, with_color=False).color is None
    vol.tsdf.fill_(0.25)
    vol.weight.fill_(3)
    vol.color.fill_(0.5)
    tsdf = vol.tsdf
    vol.reset()
    assert vol.tsdf is tsdf and bool((vol.tsdf == 1).all()) and not vol.weight.any() and not vol.color.any()


@pytest.mark.parametrize("kwargs,text", [
    (dict(origin=(0, 0)), "origin must be three numbers"),
    (dict(origin=(0, float("nan"), 0)), "origin must be three numbers"),
    (dict(dims=(4, 4)), r"dims must be \(nx, ny, nz\)"),
    (dict(dims=(4, 0, 4)), r"dims must be \(nx, ny, nz\)"),
    (dict(dims=(4, 4, 65536)), "nz <= 65535"),
    (dict(voxel_size=0.0), "voxel_size must be > 0"),
    (dict(voxel_size=float("inf")), "voxel_size must be > 0"),
    (dict(sdf_trunc=-1.0), "sdf_trunc must be > 0"),
    (dict(max_weight=0.0), "max_weight must be > 0"),
])
def test_volume_refuses_bad_parameters(kwargs, text):
    args = dict(origin=(0, 0, 0), voxel_size=0.1, dims=(4, 4, 4))
    args.update(kwargs)
    with pytest.raises(RuntimeError, match=text):
        mesh.TSDFVolume(**args)


def test_integrate_refuses_by_name_before_any_device_call():
    vol = mesh.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4))
    grey = mesh.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), with_color=False)
    C, H, W = 2, 5, 6
    d, M, K, im = torch.ones(C, H, W), torch.eye(4).repeat(C, 1, 1), torch.eye(3).repeat(C, 1, 1), torch.zeros(C, H, W, 3)
    cam = types.SimpleNamespace(K=K[0])
    for args, kw, text in (
            ((d[0], M, K, im), {}, r"depths must be a tensor \[C, H, W\]"),
            ((None, M, K, im), {}, r"depths must be a tensor \[C, H, W\]"),
            ((d, M[:1], K, im), {}, r"cameras_T_world must be \[2, 4, 4\]"),
            ((d, M, K[:, :2], im), {}, r"Ks must be \[2, 3, 3\]"),
            ((d, M, K, None), {}, "images go with a coloured volume"),
            ((d, M, K, im[:, :, :, :2]), {}, r"images must be \[2, 5, 6, 3\]"),
            ((d, M, K, im[:1]), {}, r"images must be \[2, 5, 6, 3\]"),
            ((d.double(), M, K, im), {}, "depths must be float32"),
            ((d, M.double(), K, im), {}, "cameras_T_world must be float32"),
            ((d, M, K.half(), im), {}, "Ks must be float32"),
            ((d, M, K, im.double()), {}, "images must be float32"),
            ((d, M, K, im), dict(camera_model="orthographic"), "camera_model must be one of"),
            ((d, M, K, im), dict(near_thresh=float("nan")), "must be numbers"),
            ((d, M, K, im), {}, "the volume must be on a GPU device")):   # everything else in order: no CPU path
        with pytest.raises(RuntimeError, match=text):
            vol.integrate_views(*args, **kw)
    with pytest.raises(RuntimeError, match="images go with a coloured volume"):
        grey.integrate_views(d, M, K, im)
    for args, text in (((d, M[0], cam, im[0]), r"depth must be a tensor \[H, W\]"),
                       ((d[0], M, cam, im[0]), r"camera_T_world must be \[4, 4\]"),
                       ((d[0], M[0], types.SimpleNamespace(K=None), im[0]), r"camera.K must be a tensor \[3, 3\]"),
                       ((d[0], M[0], cam, im), r"image must be a tensor \[H, W, 3\]"),
                       ((d[0], M[0], cam, im[0]), "the volume must be on a GPU device")):
        with pytest.raises(RuntimeError, match=text):
            vol.integrate(*args)
    # the volume's own tensors are the caller's to replace, and are checked
    vol.weight = vol.weight.double()
    with pytest.raises(RuntimeError, match="volume.weight must be a contiguous float32"):
        vol.integrate_views(d, M, K, im)
    assert bool((vol.tsdf == 1).all())


def test_extract_and_integrate_frame_refuse_by_name():
    vol = mesh.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4))
    with pytest.raises(RuntimeError, match="min_weight must be > 0"):
        vol.extract_mesh(min_weight=0.0)
    with pytest.raises(RuntimeError, match="level must be a number"):
        vol.extract_mesh(level=float("nan"))
    with pytest.raises(RuntimeError, match="the volume must be on a GPU device"):
        vol.extract_mesh()
    vol.tsdf = vol.tsdf[:, :, :2]
    with pytest.raises(RuntimeError, match="volume.tsdf must be a contiguous float32"):
        vol.extract_mesh()
    with pytest.raises(RuntimeError, match="depth must be 'median' or 'expected'"):
        mesh.integrate_frame(vol, None, None, None, 0.2, 100.0, 0.15, 3.0, None, depth="mean")
    with pytest.raises(RuntimeError, match="volume must be a TSDFVolume"):
        mesh.integrate_frame(None, None, None, None, 0.2, 100.0, 0.15, 3.0, None)


def read_ply(path):
    """a reader for what save_ply writes, from the header alone -> vertices, faces, colors or None"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, cur = {}, {}, None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            cur = w[1]
            counts[cur], props[cur] = int(w[2]), []
        elif w[:1] == ["property"]:
            props[cur].append(tuple(w[1:]))
    assert list(counts) == ["vertex", "face"]
    assert props["face"] == [("list", "uchar", "int", "vertex_indices")]
    names = [p[-1] for p in props["vertex"]]
    fmt = "<" + "".join({"float": "f", "uchar": "B"}[p[0]] for p in props["vertex"])
    pos, verts = end, []
    for _ in range(counts["vertex"]):
        verts.append(struct.unpack_from(fmt, data, pos))
        pos += struct.calcsize(fmt)
    faces = []
    for _ in range(counts["face"]):
        (n,) = struct.unpack_from("<B", data, pos)
        assert n == 3
        faces.append(struct.unpack_from("<3i", data, pos + 1))
        pos += 13
    assert pos == len(data)
    verts = np.array(verts, dtype=np.float64).reshape(-1, len(names))
    assert names[:3] == ["x", "y", "z"]
    colors = None
    if len(names) > 3:
        assert names[3:] == ["red", "green", "blue"]
        colors = verts[:, 3:].astype(np.uint8)
    return verts[:, :3].astype(np.float32), np.array(faces, dtype=np.int32).reshape(-1, 3), colors


def test_save_ply_round_trip(tmp_path):
    gen = torch.Generator().manual_seed(2)
    v = torch.randn(11, 3, generator=gen)
    f = torch.randint(0, 11, (7, 3), generator=gen, dtype=torch.int32)
    c = torch.rand(11, 3, generator=gen) * 1.4 - 0.2   # some outside [0, 1]: clamped
    c[0] = torch.tensor([0.0, 1.0, 0.5])
    path = tmp_path / "mesh.ply"
    mesh.save_ply(path, v, f, c)
    gv, gf, gc = read_ply(path)
    assert np.array_equal(gv, v.numpy()) and np.array_equal(gf, f.numpy())
    want = np.floor(np.clip(c.numpy().astype(np.float64), 0, 1) * 255 + 0.5).astype(np.uint8)
    assert np.abs(gc.astype(int) - want.astype(int)).max() <= 1   # fp32 rounding at a half-way value
    assert tuple(gc[0]) == (0, 255, 128) and gc.min() == 0 and gc.max() == 255
    # without colours, numpy arrays, an empty mesh
    mesh.save_ply(path, v.numpy(), f.numpy())
    gv, gf, gc = read_ply(path)
    assert np.array_equal(gv, v.numpy()) and np.array_equal(gf, f.numpy()) and gc is None
    mesh.save_ply(path, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3))
    gv, gf, gc = read_ply(path)
    assert gv.shape == (0, 3) and gf.shape == (0, 3)
    with pytest.raises(RuntimeError, match=r"vertices must be \[Nv, 3\]"):
        mesh.save_ply(path, torch.zeros(4, 2), f)
    with pytest.raises(RuntimeError, match="colors must match vertices"):
        mesh.save_ply(path, v, f, c[:5])
