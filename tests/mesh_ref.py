"""Test infrastructure: the two definitions of include/gsplat_hip.h "TSDF fusion and mesh extraction" (ABI 24) restated
in plain numpy in a chosen dtype -- float64 is the reference, the float32 run of the same text is the error envelope --
plus the inputs of tests/test_gpu_mesh.py, its left-out rule and the mesh properties both test files assert.

The triangulation's case table is NOT copied from csrc/tsdf.hip: it is derived here from the geometry (the corners of
each Kuhn tetrahedron, the rule "pr, ps, qs, qr split along pr - qs" for the two-inside quad, and the orientation from
the sign of a triple product), so the kernel's table and parity rule are checked against an independent statement."""
import functools
import itertools

import numpy as np

DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))   # edge direction e = 0..6
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))             # tetrahedron q: axes (a, b, c)
LEFT_OUT_CAP = 0.01
BAND = 2.0 ** -10


def tet_corners(q):
    """the four corners of tetrahedron q as (dx, dy, dz) offsets: 000, e_a, e_a + e_b, 111"""
    a, b, _ = PERMS[q]
    v1 = [0, 0, 0]
    v1[a] = 1
    v2 = list(v1)
    v2[b] = 1
    return ((0, 0, 0), tuple(v1), tuple(v2), (1, 1, 1))


@functools.lru_cache(maxsize=None)
def case_table():
    """{(q, m): [((i, j), (i, j), (i, j)), ...]}: the triangles of tetrahedron q whose inside corners are the bits of m,
    each a triple of tetrahedron edges (corner pairs i < j), wound so that the normal points from inside to outside;
    the winding is decided by geometry, with every edge cut at its middle"""
    table = {}
    for q in range(6):
        P = np.array(tet_corners(q), dtype=np.float64)
        for m in range(1, 15):
            ins = [i for i in range(4) if m >> i & 1]
            out = [i for i in range(4) if not m >> i & 1]
            E = lambda i, j: (min(i, j), max(i, j))
            if len(ins) == 1:
                tris = [[E(ins[0], r) for r in out]]
            elif len(ins) == 3:
                tris = [[E(out[0], r) for r in ins]]
            else:
                (p, qq), (r, s) = ins, out
                pr, ps, qs, qr = E(p, r), E(p, s), E(qq, s), E(qq, r)
                tris = [[pr, ps, qs], [pr, qs, qr]]
            towards = P[out].mean(0) - P[ins].mean(0)
            done = []
            for t in tris:
                mid = [(P[i] + P[j]) / 2 for i, j in t]
                nrm = np.cross(mid[1] - mid[0], mid[2] - mid[0])
                assert abs(nrm @ towards) > 1e-9
                done.append(tuple(t) if nrm @ towards > 0 else (t[0], t[2], t[1]))
            table[q, m] = done
    return table


# ---- integration --------------------------------------------------------------------------------------------------------
def node_positions(origin, voxel_size, dims, dt):
    """-> x [nx], y [ny], z [nz]: origin + voxel_size * index, origin and voxel_size being float32 values"""
    o = np.asarray(origin, dtype=np.float32).astype(dt)
    vs = dt(np.float32(voxel_size))
    return tuple(o[a] + vs * np.arange(dims[a]).astype(dt) for a in range(3))


def project(c0, c1, c2, K, fisheye):
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if not fisheye:
        return fx * c0 / c2 + cx, fy * c1 / c2 + cy
    r2 = c0 * c0 + c1 * c1
    r = np.sqrt(r2)
    s = np.where(r2 > 0, np.arctan2(r, c2) / np.where(r2 > 0, r, 1), 1 / c2)
    return fx * s * c0 + cx, fy * s * c1 + cy


def integrate_ref(state, depth, image, cams, Ks, fisheye, near, sdf_trunc, max_weight, depth_max, origin, voxel_size,
                  dims, dt, want_left_out=False):
    """state: (tsdf [nz,ny,nx], weight, color [nz,ny,nx,3] or None) -> the same after the C views, in dtype dt; with
    want_left_out also the [nz,ny,nx] mask of the left-out rule (meaningful for dt = float64)"""
    nx, ny, nz = dims
    tsdf, weight = state[0].astype(dt), state[1].astype(dt)
    color = None if state[2] is None else state[2].astype(dt)
    x, y, z = node_positions(origin, voxel_size, dims, dt)
    X, Y, Z = x[None, None, :], y[None, :, None], z[:, None, None]
    near, trunc, max_w, dmax = dt(np.float32(near)), dt(np.float32(sdf_trunc)), dt(np.float32(max_weight)), dt(np.float32(depth_max))
    left = np.zeros((nz, ny, nx), dtype=bool)
    C, H, W = depth.shape
    with np.errstate(all="ignore"):
        for c in range(C):
            M, K = cams[c].astype(dt), Ks[c].astype(dt)
            c0 = M[0, 0] * X + M[0, 1] * Y + M[0, 2] * Z + M[0, 3]
            c1 = M[1, 0] * X + M[1, 1] * Y + M[1, 2] * Z + M[1, 3]
            c2 = M[2, 0] * X + M[2, 1] * Y + M[2, 2] * Z + M[2, 3]
            ok = c2 > near
            u, v = project(c0, c1, c2, K, fisheye)
            uh, vh = u + dt(0.5), v + dt(0.5)
            fu, fv = np.floor(uh), np.floor(vh)
            ok = ok & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            pu = np.where(ok, fu, 0).astype(np.int64)
            pv = np.where(ok, fv, 0).astype(np.int64)
            d = depth[c].astype(dt)[pv, pu]
            ok = ok & (d > 0) & np.isfinite(d) & (d <= dmax)
            dist = np.sqrt(c0 * c0 + c1 * c1 + c2 * c2)
            sdf = (d - c2) * (dist / c2)
            ok = ok & (sdf >= -trunc)
            t = np.minimum(dt(1), sdf / trunc)
            w1 = weight + dt(1)
            tsdf = np.where(ok, (tsdf * weight + t) / w1, tsdf)
            if color is not None:
                rgb = image[c].astype(dt)[pv, pu]
                color = np.where(ok[..., None], (color * weight[..., None] + rgb) / w1[..., None], color)
            weight = np.where(ok, np.minimum(w1, max_w), weight)
            if want_left_out:
                near_int = lambda a: np.abs(a - np.round(a)) < BAND
                left |= (near_int(uh) | near_int(vh) | (np.abs(sdf + trunc) < BAND * trunc) | (np.abs(c2 - near) < BAND)) \
                    & np.isfinite(uh) & np.isfinite(vh)
    return (tsdf, weight, color, left) if want_left_out else (tsdf, weight, color)


# ---- extraction ---------------------------------------------------------------------------------------------------------
def active_cells(weight, min_weight):
    """[nz-1, ny-1, nx-1] bool (an axis of one node has no cells)"""
    ok = weight >= min_weight
    nz, ny, nx = ok.shape
    a = np.ones((max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)), dtype=bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        a &= ok[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    return a


def extract_ref(tsdf, weight, color, origin, voxel_size, level, min_weight, dt):
    """-> dict(vertices [Nv,3], faces [Nf,3] int64 in the order (cell, q, triangle), colors [Nv,3] or None,
    face_cell [Nf] the linear index of each face's cell, face_case [Nf,2] its (q, m), active [nz-1,ny-1,nx-1], tet_cases the set of
    (q, m) over the tetrahedra of all active cells, m = 0 and 15 included)"""
    nz, ny, nx = tsdf.shape
    f = tsdf.astype(dt) - dt(np.float32(level))
    inside = f < 0
    act = active_cells(weight, np.float32(min_weight))
    N = nx * ny * nz
    lin = np.arange(N).reshape(nz, ny, nx)
    # has[n, e]: edge e of node n lies in an active cell and its ends differ in sign
    in_active = np.zeros((nz, ny, nx, 7), dtype=bool)
    for e, d in enumerate(DIRS):
        for o in itertools.product((0, 1), repeat=3):             # the edge starts at corner o of the cell
            if any(o[a] + d[a] > 1 for a in range(3)):
                continue
            in_active[o[2]:nz - 1 + o[2], o[1]:ny - 1 + o[1], o[0]:nx - 1 + o[0], e] |= act
    has = np.zeros_like(in_active)
    other = np.zeros((nz, ny, nx, 7), dtype=np.int64)
    for e, (dx, dy, dz) in enumerate(DIRS):
        a = inside[:nz - dz, :ny - dy, :nx - dx]
        b = inside[dz:, dy:, dx:]
        has[:nz - dz, :ny - dy, :nx - dx, e] = (a != b) & in_active[:nz - dz, :ny - dy, :nx - dx, e]
        other[:nz - dz, :ny - dy, :nx - dx, e] = lin[dz:, dy:, dx:]
    flat = has.reshape(-1)
    vid = np.cumsum(flat) - flat                                   # ascending (n, e)
    vid = np.where(flat, vid, -1).reshape(nz, ny, nx, 7)
    n_idx, e_idx = np.nonzero(has.reshape(N, 7))
    b_idx = other.reshape(N, 7)[n_idx, e_idx]
    ff = f.reshape(-1)
    with np.errstate(all="ignore"):
        s = ff[n_idx] / (ff[n_idx] - ff[b_idx])
    ijk = np.stack([n_idx % nx, (n_idx // nx) % ny, n_idx // (nx * ny)], 1).astype(dt)
    o = np.asarray(origin, dtype=np.float32).astype(dt)
    vs = dt(np.float32(voxel_size))
    vertices = o[None, :] + vs * (ijk + s[:, None] * np.asarray(DIRS, dtype=dt)[e_idx])
    colors = None
    if color is not None:
        cc = color.astype(dt).reshape(N, 3)
        colors = cc[n_idx] + s[:, None] * (cc[b_idx] - cc[n_idx])
    # faces
    table = case_table()
    e_of = {d: e for e, d in enumerate(DIRS)}
    rows = []
    tet_cases = set()
    cz, cy, cx = np.nonzero(act)
    for q in range(6):
        P = tet_corners(q)
        m = np.zeros(len(cz), dtype=np.int64)
        for i, (dx, dy, dz) in enumerate(P):
            m |= inside[cz + dz, cy + dy, cx + dx].astype(np.int64) << i
        tet_cases |= {(q, int(c)) for c in np.unique(m)}
        for case in range(1, 15):
            sel = np.nonzero(m == case)[0]
            if not len(sel):
                continue
            for t, tri in enumerate(table[q, case]):
                ids = []
                for i, j in tri:
                    d = tuple(P[j][a] - P[i][a] for a in range(3))
                    ids.append(vid[cz[sel] + P[i][2], cy[sel] + P[i][1], cx[sel] + P[i][0], e_of[d]])
                cell = lin[cz[sel], cy[sel], cx[sel]]
                rows.append(np.stack([cell, np.full_like(cell, q), np.full_like(cell, t), np.full_like(cell, case)]
                                     + ids, 1))
    rows = np.concatenate(rows, 0) if rows else np.zeros((0, 7), dtype=np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    assert (rows[:, 4:] >= 0).all(), "a face uses an edge that carries no vertex"
    return dict(vertices=vertices, faces=rows[:, 4:], colors=colors, face_cell=rows[:, 0], face_case=rows[:, [1, 3]],
                active=act, tet_cases=tet_cases)


# ---- mesh properties ----------------------------------------------------------------------------------------------------
def canonical_faces(faces):
    """each face rotated to its smallest index first, then the rows sorted"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    k = np.argmin(faces, 1)
    rot = np.stack([faces[np.arange(len(faces)), (k + i) % 3] for i in range(3)], 1)
    return rot[np.lexsort((rot[:, 2], rot[:, 1], rot[:, 0]))]


def directed_edges(faces):
    faces = np.asarray(faces, dtype=np.int64)
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0)


def is_closed_manifold(faces):
    """every directed edge appears once and its reverse once"""
    e = directed_edges(faces)
    n = int(e.max()) + 1
    key, rev = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    return bool((counts == 1).all()) and bool(np.isin(rev, uniq).all())


def interior_edges_are_paired(faces):
    """no directed edge twice (an open mesh: an edge and its reverse at most once each)"""
    e = directed_edges(faces)
    n = int(e.max()) + 1
    _, counts = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    return bool((counts == 1).all())


def euler_characteristic(n_vertices, faces):
    e = np.sort(directed_edges(faces), 1)
    return n_vertices - len(np.unique(e, axis=0)) + len(faces)


def face_normals_and_centroids(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), v.mean(1)


# ---- analytic volumes ---------------------------------------------------------------------------------------------------
SPHERE = dict(dims=(19, 17, 13), centre=(9.3, 8.1, 6.2), radius=4.7)


def sphere_volume():
    """the signed distance of SPHERE on unit nodes at the origin, as float32 -> tsdf [nz,ny,nx], weight, color"""
    nx, ny, nz = SPHERE["dims"]
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c = SPHERE["centre"]
    tsdf = (np.sqrt((x - c[0]) ** 2.0 + (y - c[1]) ** 2.0 + (z - c[2]) ** 2.0) - SPHERE["radius"]).astype(np.float32)
    color = np.stack([x / nx, y / ny, z / nz], -1).astype(np.float32)
    return tsdf, np.ones_like(tsdf), color


def sphere_radial_bound():
    """linear interpolation along an edge of length <= L = sqrt(3) h of the distance to a sphere: L^2 / (8 (R - L))"""
    L = np.sqrt(3.0)
    return L * L / (8 * (SPHERE["radius"] - L))


PLANE = dict(dims=(11, 9, 8), normal=(0.48, -0.6, 0.64), offset=3.1)


def plane_volume():
    nx, ny, nz = PLANE["dims"]
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    n = PLANE["normal"]
    tsdf = (n[0] * x + n[1] * y + n[2] * z - PLANE["offset"]).astype(np.float32)
    return tsdf, np.ones_like(tsdf), None


def random_volume(dims=(9, 7, 6), seed=5, hole_share=0.2):
    """random tsdf in [-1, 1], a random share of the weights zero, random colour.  The holes are 2 x 2 x 2 blocks at random
    places, punched until the share is reached: single random nodes would leave one cell in six active, too few to show
    every sign case in every tetrahedron"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    tsdf = rng.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    weight = np.full((nz, ny, nx), 2.0, dtype=np.float32)
    while (weight == 0).mean() < hole_share:
        k, j, i = rng.integers(0, nz - 1), rng.integers(0, ny - 1), rng.integers(0, nx - 1)
        weight[k:k + 2, j:j + 2, i:i + 2] = 0
    color = rng.uniform(0, 1, (nz, ny, nx, 3)).astype(np.float32)
    return tsdf, weight, color


# ---- the integration cases of tests/test_gpu_mesh.py ---------------------------------------------------------------------
VOLUMES = {"24x20x16": (24, 20, 16), "65x9x5": (65, 9, 5)}
VOXEL = 0.05
FRAME = (70, 45)
NEAR, DEPTH_MAX, MAX_WEIGHT = 0.2, 4.0, 64.0
SDF_TRUNC = 4 * VOXEL


def view_camera(yaw=0.3, shift=(0.0, 0.0, 0.0)):
    """-> camera_T_world [4,4], K [3,3] float32: fx = fy = 60, an offset principal point, a yaw about y"""
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = np.array([0.07, -0.04, 1.35]) + np.asarray(shift)
    K = np.array([[60.0, 0, 33.7], [0, 60.0, 23.2], [0, 0, 1]])
    return M.astype(np.float32), K.astype(np.float32)


def volume_origin(dims):
    """the volume centred on the world origin"""
    return tuple(np.float32(-0.5 * VOXEL * (n - 1)) for n in dims)


def view_depth(M, K, fisheye, radius=0.3, plane_z=1.75):
    """the camera-frame z of an analytic sphere at the world origin in front of the plane z_cam = plane_z, seen through
    (M, K), with patches of invalid values: 0, negative, NaN, beyond DEPTH_MAX, +inf -> depth [H,W], image [H,W,3]"""
    W, H = FRAME
    M, K = M.astype(np.float64), K.astype(np.float64)
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a, b = (px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1]
    if fisheye:
        th = np.sqrt(a * a + b * b)
        k = np.where(th > 0, np.tan(th) / np.where(th > 0, th, 1), 1.0)
        a, b = a * k, b * k
    ray = np.stack([a, b, np.ones_like(a)], -1)                   # camera-frame ray with z = 1
    centre = M[:3, 3]                                             # the world origin in the camera frame
    A = (ray * ray).sum(-1)
    B = ray @ centre
    disc = B * B - A * (centre @ centre - radius * radius)
    z_sphere = (B - np.sqrt(np.maximum(disc, 0))) / A
    depth = np.where(disc > 0, z_sphere, plane_z)
    depth[3:7, 5:11] = 0.0
    depth[10:13, 40:47] = -1.0
    depth[30:34, 20:26] = np.nan
    depth[36:41, 50:60] = DEPTH_MAX + 1.0
    depth[20:22, 60:64] = np.inf
    rng = np.random.default_rng(17)
    return depth.astype(np.float32), rng.uniform(0, 1, (H, W, 3)).astype(np.float32)


def start_state(dims, seed=3):
    """a volume that already holds something: random tsdf, integer weights 0..5 (a third of them 0, where tsdf is 1 and
    the colour 0 as in a fresh volume), random colour"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    weight = np.maximum(rng.integers(-2, 6, (nz, ny, nx)), 0).astype(np.float32)
    tsdf = np.where(weight > 0, rng.uniform(-1, 1, (nz, ny, nx)), 1.0).astype(np.float32)
    color = np.where(weight[..., None] > 0, rng.uniform(0, 1, (nz, ny, nx, 3)), 0.0).astype(np.float32)
    return tsdf, weight, color


@functools.lru_cache(maxsize=None)
def integration_case(volume, fisheye):
    """computed once per case and shared, never modified -> dict(dims, origin, depth [1,H,W], image, cams, Ks, start,
    f64, f32 (tsdf, weight, color), left_out)"""
    dims = VOLUMES[volume]
    M, K = view_camera()
    depth, image = view_depth(M, K, fisheye)
    cams, Ks, depth, image = M[None], K[None], depth[None], image[None]
    origin = volume_origin(dims)
    start = start_state(dims)
    args = (depth, image, cams, Ks, fisheye, NEAR, SDF_TRUNC, MAX_WEIGHT, DEPTH_MAX, origin, VOXEL, dims)
    *f64, left = integrate_ref(start, *args, np.float64, want_left_out=True)
    f32 = integrate_ref(start, *args, np.float32)
    return dict(dims=dims, origin=origin, depth=depth, image=image, cams=cams, Ks=Ks, start=start, f64=tuple(f64),
                f32=f32, left_out=left)
