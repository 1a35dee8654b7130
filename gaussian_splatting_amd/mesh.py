"""Depth maps to a triangle mesh over the C ABI (csrc/tsdf.hip): TSDF fusion and marching tetrahedra.

What 2DGS and its successors do after training: render a depth map from every training view, fuse the maps into a
truncated signed distance volume, triangulate its zero level set.

    TSDFVolume(origin, voxel_size, dims)    the volume: tsdf, weight, color as plain tensors
      .integrate(depth, camera_T_world, camera, image)       one view
      .integrate_views(depths, cameras_T_world, Ks, images)  a batch in one launch: the volume moves once per batch
      .extract_mesh()                                        -> vertices [Nv, 3], faces [Nf, 3] int32, colors [Nv, 3] or None
    integrate_frame(volume, gaussians, camera_T_world, camera, ...)   render with fused.rasterize_median_depth and fuse
    save_ply(path, vertices, faces, colors)                           binary little-endian PLY (host code)

        vol = mesh.TSDFVolume(origin=(-2, -2, -2), voxel_size=4 / 255, dims=(256, 256, 256), device="cuda")
        for camera_T_world, camera in train_views:
            mesh.integrate_frame(vol, gaussians, camera_T_world, camera, 0.2, 100.0, 100, 3.0, background)
        mesh.save_ply("scene.ply", *vol.extract_mesh())

The definitions are in include/gsplat_hip.h (ABI 24), the reasoning in DESIGN.md 7o.  The signed distance is taken along
the viewing ray (Open3D and 2DGS take the plain z difference; the two agree on the optical axis).  The extraction has no
atomics: the same volume gives the same bits.
"""
import math

import numpy as np
import torch

from . import _hip

CAMERA_MODELS = ("pinhole", "fisheye")
_INT32_MAX = 2 ** 31 - 1


def _require(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _mode(camera_model):
    _require(camera_model in CAMERA_MODELS, f"camera_model must be one of {' / '.join(repr(m) for m in CAMERA_MODELS)}, "
                                            f"got {camera_model!r}")
    return _hip.GS_RASTER_FISHEYE if camera_model == "fisheye" else _hip.GS_RASTER_CLASSIC


class TSDFVolume:
    """nx x ny x nz nodes, node (i, j, k) at origin + voxel_size (i, j, k) in world coordinates.

    tsdf, weight [nz, ny, nx] and color [nz, ny, nx, 3] (None with with_color=False) are plain float32 tensors on
    `device`: fresh they hold 1, 0 and 0.  sdf_trunc=None means 4 voxel_size; max_weight caps the running average's
    weight, so that a long capture keeps following its later views."""

    def __init__(self, origin, voxel_size, dims, sdf_trunc=None, with_color=True, max_weight=64.0, device=None):
        origin = tuple(float(x) for x in origin)
        dims = tuple(int(n) for n in dims)
        voxel_size = float(voxel_size)
        _require(len(origin) == 3 and all(math.isfinite(x) for x in origin), f"TSDFVolume: origin must be three numbers, got {origin}")
        _require(len(dims) == 3 and min(dims) >= 1, f"TSDFVolume: dims must be (nx, ny, nz), each at least 1, got {dims}")
        _require(dims[1] <= 262140 and dims[2] <= 65535, f"TSDFVolume: ny <= 262140 and nz <= 65535, got {dims}")
        _require(math.isfinite(voxel_size) and voxel_size > 0, f"TSDFVolume: voxel_size must be > 0, got {voxel_size}")
        sdf_trunc = 4.0 * voxel_size if sdf_trunc is None else float(sdf_trunc)
        _require(math.isfinite(sdf_trunc) and sdf_trunc > 0, f"TSDFVolume: sdf_trunc must be > 0, got {sdf_trunc}")
        max_weight = float(max_weight)
        _require(max_weight > 0, f"TSDFVolume: max_weight must be > 0, got {max_weight}")
        self.origin, self.voxel_size, self.dims = origin, voxel_size, dims
        self.sdf_trunc, self.max_weight = sdf_trunc, max_weight
        nx, ny, nz = dims
        self.tsdf = torch.ones(nz, ny, nx, dtype=torch.float32, device=device)
        self.weight = torch.zeros(nz, ny, nx, dtype=torch.float32, device=device)
        self.color = torch.zeros(nz, ny, nx, 3, dtype=torch.float32, device=device) if with_color else None

    @property
    def device(self):
        return self.tsdf.device

    def reset(self):
        """back to the fresh volume, in place"""
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def _check_state(self, who):
        nx, ny, nz = self.dims
        for name, t, shape in (("tsdf", self.tsdf, (nz, ny, nx)), ("weight", self.weight, (nz, ny, nx)),
                               ("color", self.color, (nz, ny, nx, 3))):
            if t is None and name == "color":
                continue
            _require(torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()
                     and t.device == self.tsdf.device and not t.requires_grad,
                     f"{who}: volume.{name} must be a contiguous float32 {list(shape)} on the volume's device without a gradient")
        _require(self.tsdf.is_cuda, f"{who}: the volume must be on a GPU device (no CPU path)")

    # ---- fusion -------------------------------------------------------------------------------------------------------
    def integrate_views(self, depths, cameras_T_world, Ks, images=None, camera_model="pinhole", near_thresh=0.2,
                        depth_max=math.inf):
        """fuse C views of one size in one launch, in the order given (gs_tsdf_integrate): depths [C, H, W] camera-frame
        z (fused.rasterize_median_depth's median_depth, or depth / alpha), <= 0 / not finite / > depth_max where there is
        nothing to fuse; cameras_T_world [C, 4, 4], Ks [C, 3, 3]; images [C, H, W, 3] iff the volume has colour.  float32
        on the volume's device, else RuntimeError before any device call.  The result is that of C single-view calls,
        bit for bit."""
        who = "TSDFVolume.integrate_views"
        mode = _mode(camera_model)
        _require(torch.is_tensor(depths) and depths.dim() == 3, f"{who}: depths must be a tensor [C, H, W]")
        C, H, W = (int(s) for s in depths.shape)
        _require(torch.is_tensor(cameras_T_world) and tuple(cameras_T_world.shape) == (C, 4, 4),
                 f"{who}: cameras_T_world must be [{C}, 4, 4], one per view")
        _require(torch.is_tensor(Ks) and tuple(Ks.shape) == (C, 3, 3), f"{who}: Ks must be [{C}, 3, 3], one per view")
        _require((images is None) == (self.color is None),
                 f"{who}: images go with a coloured volume: give them iff the volume was made with_color")
        named = [("depths", depths), ("cameras_T_world", cameras_T_world), ("Ks", Ks)]
        if images is not None:
            _require(torch.is_tensor(images) and tuple(images.shape) == (C, H, W, 3), f"{who}: images must be [{C}, {H}, {W}, 3]")
            named.append(("images", images))
        for name, t in named:
            _require(t.dtype == torch.float32 and t.device == self.tsdf.device,
                     f"{who}: {name} must be float32 on the volume's device")
        near_thresh, depth_max = float(near_thresh), float(depth_max)
        _require(near_thresh == near_thresh and depth_max == depth_max, f"{who}: near_thresh and depth_max must be numbers")
        self._check_state(who)
        p = _hip.ptr
        with torch.no_grad():
            keep = [t.detach().contiguous() for _, t in named]
            _hip.call("gs_tsdf_integrate", p(keep[0]), p(keep[3]) if images is not None else None, p(keep[1]), p(keep[2]),
                      C, W, H, mode, near_thresh, self.sdf_trunc, self.max_weight, depth_max, *self.origin, self.voxel_size,
                      *self.dims, p(self.tsdf), p(self.weight), p(self.color), _hip.current_stream())
        return self

    def integrate(self, depth, camera_T_world, camera, image=None, camera_model="pinhole", near_thresh=0.2,
                  depth_max=math.inf):
        """fuse one view: depth [H, W], camera_T_world [4, 4], camera.K [3, 3], image [H, W, 3] iff the volume has colour"""
        who = "TSDFVolume.integrate"
        _require(torch.is_tensor(depth) and depth.dim() == 2, f"{who}: depth must be a tensor [H, W]")
        _require(torch.is_tensor(camera_T_world) and tuple(camera_T_world.shape) == (4, 4), f"{who}: camera_T_world must be [4, 4]")
        K = getattr(camera, "K", None)
        _require(torch.is_tensor(K) and tuple(K.shape) == (3, 3), f"{who}: camera.K must be a tensor [3, 3]")
        if image is not None:
            _require(torch.is_tensor(image) and image.dim() == 3, f"{who}: image must be a tensor [H, W, 3]")
            image = image[None]
        return self.integrate_views(depth[None], camera_T_world[None], K[None], image, camera_model, near_thresh, depth_max)

    # ---- extraction ---------------------------------------------------------------------------------------------------
    def extract_mesh(self, level=0.0, min_weight=1.0):
        """-> vertices [Nv, 3] float32, faces [Nf, 3] int32, colors [Nv, 3] float32 or None: the level set tsdf = level by
        marching tetrahedra over the cells whose 8 corners all have weight >= min_weight.  Every face's normal points
        towards positive tsdf (free space, the cameras); the mesh is watertight wherever observed cells meet.  An empty
        mesh is tensors with zero rows.  Two passes with a scan between them; the totals are read on the host once."""
        who = "TSDFVolume.extract_mesh"
        level, min_weight = float(level), float(min_weight)
        _require(level == level, f"{who}: level must be a number")
        _require(min_weight > 0, f"{who}: min_weight must be > 0, got {min_weight}")
        self._check_state(who)
        dev = self.tsdf.device
        nx, ny, nz = self.dims
        N = nx * ny * nz
        p, lib = _hip.ptr, _hip.lib()
        with torch.no_grad():
            ws = torch.empty(max(lib.gs_tsdf_extract_workspace_bytes(nx, ny, nz), 1), dtype=torch.uint8, device=dev)
            edge_mask = torch.empty(N, dtype=torch.uint8, device=dev)
            vert_count = torch.empty(N, dtype=torch.int32, device=dev)
            face_count = torch.empty(N, dtype=torch.int32, device=dev)
            _hip.call("gs_tsdf_extract_count", p(self.tsdf), p(self.weight), nx, ny, nz, level, min_weight, p(ws), p(edge_mask),
                      p(vert_count), p(face_count), _hip.current_stream())
            vert_end = torch.cumsum(vert_count, 0, dtype=torch.int64)
            face_end = torch.cumsum(face_count, 0, dtype=torch.int64)
            n_vert, n_face = (int(x) for x in torch.stack((vert_end[-1], face_end[-1])).cpu())
            _require(n_vert <= _INT32_MAX and n_face <= _INT32_MAX,
                     f"{who}: {n_vert} vertices and {n_face} faces do not fit int32 indices; extract the volume in parts")
            vertices = torch.empty(n_vert, 3, dtype=torch.float32, device=dev)
            faces = torch.empty(n_face, 3, dtype=torch.int32, device=dev)
            colors = torch.empty(n_vert, 3, dtype=torch.float32, device=dev) if self.color is not None else None
            if n_vert == 0 and n_face == 0:
                return vertices, faces, colors
            vert_offset = (vert_end - vert_count).to(torch.int32)
            face_offset = (face_end - face_count).to(torch.int32)
            _hip.call("gs_tsdf_extract_emit", p(self.tsdf), p(self.color), p(edge_mask), p(vert_offset), p(face_offset),
                      p(face_count), nx, ny, nz, level, *self.origin, self.voxel_size, p(vertices), p(colors), p(faces),
                      _hip.current_stream())
        return vertices, faces, colors


def integrate_frame(volume, gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist,
                    background_rgb, depth="median", min_alpha=0.5, **rasterize_keywords):
    """render one view of the Gaussians with fused.rasterize_median_depth and fuse its depth map and image into the volume.

    depth="median": the median depth (2DGS's depth_ratio = 1, what 2DGS meshes bounded scenes with); depth="expected":
    depth / alpha.  Pixels with alpha < min_alpha are left out.  rasterize_keywords go to the renderer (antialiased,
    camera_model, filter3d); camera_model is passed on to the fusion, near_thresh is the renderer's.  Runs under
    torch.no_grad().  -> the rendered (image, depth map as fused)."""
    from . import fused

    _require(depth in ("median", "expected"), f"integrate_frame: depth must be 'median' or 'expected', got {depth!r}")
    _require(isinstance(volume, TSDFVolume), "integrate_frame: volume must be a TSDFVolume")
    with torch.no_grad():
        image, z_sum, alpha, median_depth, _, _, _ = fused.rasterize_median_depth(
            gaussians, camera_T_world, camera, near_thresh, far_thresh, cull_mask_padding, mh_dist, True, background_rgb,
            **rasterize_keywords)
        d = median_depth if depth == "median" else z_sum / alpha
        d = torch.where(alpha < min_alpha, torch.zeros_like(d), d)
        volume.integrate(d, camera_T_world, camera, image if volume.color is not None else None,
                         camera_model=rasterize_keywords.get("camera_model", "pinhole"), near_thresh=near_thresh)
    return image, d


def save_ply(path, vertices, faces, colors=None):
    """binary little-endian PLY: float x y z, uchar red green blue (colors in [0, 1], clamped) when colors is given, faces as
    `uchar int` lists.  Host code: tensors are copied to the CPU."""
    v = torch.as_tensor(vertices).detach().to("cpu", torch.float32).contiguous()
    f = torch.as_tensor(faces).detach().to("cpu", torch.int32).contiguous()
    _require(v.dim() == 2 and v.shape[1] == 3, f"save_ply: vertices must be [Nv, 3], got {list(v.shape)}")
    _require(f.dim() == 2 and f.shape[1] == 3, f"save_ply: faces must be [Nf, 3], got {list(f.shape)}")
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}", "property float x",
              "property float y", "property float z"]
    vert = v.numpy().astype("<f4")
    if colors is not None:
        c = torch.as_tensor(colors).detach().to("cpu", torch.float32)
        _require(tuple(c.shape) == tuple(v.shape), f"save_ply: colors must match vertices, got {list(c.shape)}")
        header += ["property uchar red", "property uchar green", "property uchar blue"]
        c8 = (c.clamp(0, 1) * 255 + 0.5).floor().to(torch.uint8).numpy()
        rec = np.empty(v.shape[0], dtype=[("p", "<f4", 3), ("c", "u1", 3)])
        rec["p"], rec["c"] = vert, c8
        vert = rec
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    face = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", 3)])
    face["n"], face["i"] = 3, f.numpy()
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())
