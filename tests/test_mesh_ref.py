"""The reference of the TSDF fusion and the mesh extraction (tests/mesh_ref.py) checked on its own, on the CPU: on
analytic signed-distance volumes the extracted mesh is a closed, consistently oriented manifold of the right topology
within the linear-interpolation bound; with weight holes no face touches an inactive cell and no vertex is left
unused; the left-out rule of the GPU integration test leaves out at most LEFT_OUT_CAP of the nodes; the float64
integration agrees with a node-by-node restatement in plain Python."""
import numpy as np
import pytest

from . import mesh_ref as R


def _sphere():
    tsdf, weight, color = R.sphere_volume()
    return R.extract_ref(tsdf, weight, color, (0, 0, 0), 1.0, 0.0, 1.0, np.float64)


def test_case_table_has_one_or_two_triangles_and_complements_reverse():
    table = R.case_table()
    for q in range(6):
        for m in range(1, 15):
            tris = table[q, m]
            assert len(tris) == (2 if bin(m).count("1") == 2 else 1)
            # the complementary case is the same surface seen from the other side
            a = R.canonical_faces([[e[0] * 4 + e[1] for e in t] for t in tris])
            b = R.canonical_faces([[e[0] * 4 + e[1] for e in (t[0], t[2], t[1])] for t in table[q, 15 - m]])
            if len(tris) == 1:
                assert np.array_equal(a, b)
            else:   # the quad is the same four edges, reversed (the diagonal is the reversed case's own)
                assert set(a.reshape(-1)) == set(b.reshape(-1))


def test_sphere_mesh_is_a_closed_oriented_sphere():
    m = _sphere()
    v, f = m["vertices"], m["faces"]
    print(len(v), "vertices", len(f), "faces")
    assert (len(v), len(f)) == (1228, 2452)
    assert R.is_closed_manifold(f)
    assert R.euler_characteristic(len(v), f) == 2
    nrm, cen = R.face_normals_and_centroids(v, f)
    assert (np.linalg.norm(nrm, axis=1) > 0).all(), "a face of zero area"
    grad = cen - np.asarray(R.SPHERE["centre"])
    assert ((nrm * grad).sum(1) > 0).all()
    err = np.abs(np.linalg.norm(v - np.asarray(R.SPHERE["centre"]), axis=1) - R.SPHERE["radius"])
    print("largest radial error", err.max(), "bound", R.sphere_radial_bound())
    assert err.max() <= R.sphere_radial_bound()
    assert len(np.unique(f)) == len(v)
    # colours are interpolated like positions: here colour = position / dims exactly
    want = v / np.asarray(R.SPHERE["dims"], dtype=np.float64)
    assert np.abs(m["colors"] - want).max() < 1e-6


def test_plane_mesh_is_oriented_and_paired():
    tsdf, weight, _ = R.plane_volume()
    m = R.extract_ref(tsdf, weight, None, (0.5, -1.0, 2.0), 0.25, 0.0, 1.0, np.float64)
    v, f = m["vertices"], m["faces"]
    assert len(f) > 100 and m["colors"] is None
    assert R.interior_edges_are_paired(f)
    assert R.euler_characteristic(len(v), f) == 1   # a disc
    nrm, _ = R.face_normals_and_centroids(v, f)
    assert ((nrm @ np.asarray(R.PLANE["normal"])) > 0).all()
    # linear interpolation of a linear field is exact: every vertex lies on the plane
    p = (v - np.array([0.5, -1.0, 2.0])) / 0.25
    assert np.abs(p @ np.asarray(R.PLANE["normal"]) - R.PLANE["offset"]).max() < 1e-5
    # a level other than zero moves the plane
    m2 = R.extract_ref(tsdf, weight, None, (0.5, -1.0, 2.0), 0.25, 0.5, 1.0, np.float64)
    p2 = (m2["vertices"] - np.array([0.5, -1.0, 2.0])) / 0.25
    assert np.abs(p2 @ np.asarray(R.PLANE["normal"]) - R.PLANE["offset"] - 0.5).max() < 1e-5


def test_weight_holes_leave_no_face_in_an_inactive_cell_and_no_unused_vertex():
    for tsdf, weight, color in (R.random_volume(), R.sphere_volume()):
        weight = weight.copy()
        if weight.min() > 0:   # the sphere: punch holes through its surface
            weight[3:6, 4:9, 2:5] = 0
            weight[8, 8, 10] = 0
        m = R.extract_ref(tsdf, weight, color, (0, 0, 0), 1.0, 0.0, 1.0, np.float64)
        v, f, act = m["vertices"], m["faces"], m["active"]
        assert len(f) > 0 and not act.all() and act.any()
        _, cen = R.face_normals_and_centroids(v, f)
        cell = np.floor(cen).astype(int)
        assert act[cell[:, 2], cell[:, 1], cell[:, 0]].all()
        nz, ny, nx = tsdf.shape
        assert np.array_equal((cell[:, 2] * ny + cell[:, 1]) * nx + cell[:, 0], m["face_cell"])
        assert len(np.unique(f)) == len(v)
        assert R.interior_edges_are_paired(f)


def test_random_volume_shows_every_case_in_every_tetrahedron():
    tsdf, weight, color = R.random_volume()
    m = R.extract_ref(tsdf, weight, color, (0, 0, 0), 1.0, 0.0, 1.0, np.float64)
    assert m["tet_cases"] == {(q, c) for q in range(6) for c in range(16)}
    assert {(int(q), int(c)) for q, c in m["face_case"]} == {(q, c) for q in range(6) for c in range(1, 15)}
    share = (weight == 0).mean()
    assert 0.2 <= share < 0.23
    # inactive cells next to active ones
    act = m["active"]
    assert (act[:, :, 1:] != act[:, :, :-1]).any() and (act[1:] != act[:-1]).any()


def test_float32_restatement_makes_the_same_sign_decisions():
    tsdf, weight, color = R.random_volume()
    a = R.extract_ref(tsdf, weight, color, (0, 0, 0), 1.0, 0.0, 1.0, np.float64)
    b = R.extract_ref(tsdf, weight, color, (0, 0, 0), 1.0, 0.0, 1.0, np.float32)
    assert np.array_equal(a["faces"], b["faces"])
    assert b["vertices"].dtype == np.float32 and np.abs(a["vertices"] - b["vertices"]).max() < 1e-5


def test_empty_inputs_give_empty_meshes():
    tsdf, weight, _ = R.plane_volume()
    for t, w in ((np.ones_like(tsdf), weight), (tsdf, np.zeros_like(weight)), (tsdf[:, :, :1], weight[:, :, :1])):
        m = R.extract_ref(t, w, None, (0, 0, 0), 1.0, 0.0, 1.0, np.float64)
        assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3)


@pytest.mark.parametrize("fisheye", (False, True))
@pytest.mark.parametrize("volume", tuple(R.VOLUMES))
def test_left_out_rule_leaves_out_at_most_the_cap(volume, fisheye):
    case = R.integration_case(volume, fisheye)
    share = case["left_out"].mean()
    updated = (case["f64"][1] != case["start"][1]).mean()
    print(f"{volume} fisheye={fisheye}: left out {share:.4%}, updated {updated:.1%}")
    assert share <= R.LEFT_OUT_CAP
    # the case is worth running: the view updates a good part of the volume and skips a good part
    assert 0.2 < updated < 0.95
    keep = ~case["left_out"]
    assert np.array_equal(case["f32"][1][keep], case["f64"][1][keep])


def test_integration_agrees_with_a_node_by_node_restatement():
    """the vectorised float64 reference against the issue's six steps written out for single nodes"""
    case = R.integration_case("24x20x16", False)
    nx, ny, nz = case["dims"]
    M, K = case["cams"][0].astype(np.float64), case["Ks"][0].astype(np.float64)
    depth, image = case["depth"][0].astype(np.float64), case["image"][0].astype(np.float64)
    o = np.asarray(case["origin"], dtype=np.float64)
    vs, trunc = float(np.float32(R.VOXEL)), float(np.float32(R.SDF_TRUNC))
    rng = np.random.default_rng(0)
    W, H = R.FRAME
    for n in rng.integers(0, nx * ny * nz, 400):
        i, j, k = n % nx, (n // nx) % ny, n // (nx * ny)
        t0, w0, c0 = (case["start"][a][k, j, i].astype(np.float64) for a in range(3))
        want = (t0, w0, c0)
        pc = M[:3, :3] @ (o + vs * np.array([i, j, k])) + M[:3, 3]
        if pc[2] > float(np.float32(R.NEAR)):
            u, v = K[0, 0] * pc[0] / pc[2] + K[0, 2], K[1, 1] * pc[1] / pc[2] + K[1, 2]
            px, py = int(np.floor(u + 0.5)), int(np.floor(v + 0.5))
            if 0 <= px < W and 0 <= py < H:
                d = depth[py, px]
                if d > 0 and np.isfinite(d) and d <= R.DEPTH_MAX:
                    sdf = (d - pc[2]) * np.linalg.norm(pc) / pc[2]
                    if sdf >= -trunc:
                        t = min(1.0, sdf / trunc)
                        want = ((t0 * w0 + t) / (w0 + 1), min(w0 + 1, R.MAX_WEIGHT), (c0 * w0 + image[py, px]) / (w0 + 1))
        got = tuple(case["f64"][a][k, j, i] for a in range(3))
        assert abs(got[0] - want[0]) < 1e-9 and got[1] == want[1] and np.abs(got[2] - want[2]).max() < 1e-9
