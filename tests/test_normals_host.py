"""CPU: the float64 helper of the neighbour-list / normal tests (tests/normals_ref.py) on hand-worked cases, and the
host stages of the mesh-only scan layout (scans.clean_mesh, clean_segments, the scan naming, the points table) against
numpy restatements of the reference's code on a tiny mesh with unreferenced vertices."""
import os

import numpy as np
import pytest

import dataset_cases as D
import normals_ref as N


# ------------------------------------------------------------------------------------------------------- the helper
def test_neighbour_lists_by_hand():
    # on the x axis at 0, 0.25, 0.5, -0.25 and a copy of 0.25: distances from the origin 0, .25, .5, .25, .25
    ref = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [-0.25, 0, 0], [0.25, 0, 0]], np.float32)
    q = np.zeros((1, 3), np.float32)
    idx, count = N.knn_hybrid_f64(q, ref, 6, 0.5)
    assert count.tolist() == [4] and idx.tolist() == [[0, 1, 3, 4, -1, -1]]        # 0.5 itself is not < 0.5; ties by index
    idx, count = N.knn_hybrid_f64(q, ref, 2, 0.5)
    assert count.tolist() == [2] and idx.tolist() == [[0, 1]]                      # the cut falls inside the tie
    idx, count = N.knn_hybrid_f64(q, ref, 3, 0.51)
    assert idx.tolist() == [[0, 1, 3]]
    idx, count = N.knn_hybrid_f64(q + 5, ref, 3, 0.5)
    assert count.tolist() == [0] and idx.tolist() == [[-1, -1, -1]]
    # the radius is rounded to float32 first: a point at float32(0.1) from the query has d2 == r2 and is outside
    idx, count = N.knn_hybrid_f64(np.zeros((1, 3)), np.array([[np.float32(0.1), 0, 0]]), 1, 0.1)
    assert count.tolist() == [0]
    assert N.knn_hybrid_f64(np.zeros((0, 3)), ref, 2, 0.5)[0].shape == (0, 2)


def test_pca_by_hand():
    ref = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [1, 2, 0], [0, 0, 5]], np.float32)
    q = np.array([[0.5, 1, 0], [9, 9, 9]], np.float32)
    idx = np.array([[0, 1, 2, 3], [0, 1, -1, -1]], np.int32)
    normal, lam, s = N.pca_f64(q, ref, idx, np.array([4, 2], np.int32))
    assert np.allclose(np.abs(normal[0]), [0, 0, 1]) and np.allclose(lam[0], [0, 0.25, 1.0])
    assert s[0] == 1.25                                                            # 4 neighbours at squared distance 1.25
    assert normal[1].tolist() == [0, 0, 1] and s[1] == 0 and not lam[1].any()      # fewer than 3: the default


def test_sign_rule():
    n = np.array([[0.6, -0.8, 0], [-0.6, 0.8, 0], [0.5, -0.5, 0.1], [-0.5, 0.5, 0.1], [0, 0, 1], [0, 0, -1]], np.float32)
    assert N.sign_rule_holds(n).tolist() == [False, True, True, False, True, False]


def test_case_generators_are_the_documented_shapes():
    shapes = {k: f().shape[0] for k, f in N.NORMAL_CASES.items()}
    assert shapes == {"noisy_plane": 2500, "sphere": 3000, "two_planes": 2400, "planar_lattice": 400, "slab_lattice": 432,
                      "sparse_cube": 300}
    assert N.line().shape == (200, 3) and all(f().dtype == np.float32 for f in N.NORMAL_CASES.values())


# --------------------------------------------------------------------------------------------- mesh-only host stages
def _tiny_mesh():
    """9 vertices, 3 of them (1, 4, 8) referenced by no face."""
    rng = np.random.default_rng(3)
    vertices = rng.random((9, 3)).astype(np.float32)
    colors = rng.random((9, 3)).astype(np.float32)
    faces = np.array([[0, 2, 3], [2, 3, 5], [5, 6, 7], [7, 6, 0]], np.int32)
    return vertices, colors, faces


def _clean_mesh_as_written(vertices, colors, faces):
    """pseudo_masks/datasets/arkit.py:61-84 in its own words."""
    valid_vertices = np.unique(faces)
    unreferenced = np.setdiff1d(np.arange(vertices.shape[0]), valid_vertices)
    removed = np.zeros(vertices.shape[0])
    removed[unreferenced] = 1
    updated = (faces - np.cumsum(removed)[faces]).astype(np.intc)
    return vertices[valid_vertices], colors[valid_vertices], updated


def test_clean_mesh():
    from unscene3d_amd.pseudo_masks import scans
    vertices, colors, faces = _tiny_mesh()
    v, c, f, kept = scans.clean_mesh(vertices, colors, faces)
    ev, ec, ef = _clean_mesh_as_written(vertices, colors, faces)
    assert kept.tolist() == [0, 2, 3, 5, 6, 7]
    assert np.array_equal(v, ev) and np.array_equal(c, ec) and np.array_equal(f, ef) and f.dtype == np.int32
    assert np.array_equal(v[f], vertices[faces])                                   # every face keeps its corners
    v2, _, f2, kept2 = scans.clean_mesh(v, c, f)                                   # nothing left to remove
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and kept2.tolist() == list(range(6))


def test_clean_segments():
    from unscene3d_amd.pseudo_masks import scans
    comps = np.array([4, 4, 4, 7, 7, 1, 4, 9, 9, 9])
    kept, valid = scans.clean_segments(comps, min_vert_num=3)
    ids, counts = np.unique(comps, return_counts=True)
    expect = ~np.isin(comps, ids[counts < 3])
    assert np.array_equal(valid, expect) and valid.tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 1, 1]
    assert np.array_equal(kept, comps[expect])
    assert scans.clean_segments(comps, min_vert_num=5)[1].sum() == 0 and scans.clean_segments(comps, 1)[1].all()


def test_scan_naming(tmp_path):
    from unscene3d_amd.pseudo_masks import scans
    os.makedirs(tmp_path / "41069021")
    v, c, f = _tiny_mesh()
    D.write_ply(str(tmp_path / "41069021" / "41069021_3dod_mesh.ply"), v, (c * 255).astype(np.uint8), f)
    D.write_ply(str(tmp_path / "40753679.ply"), v, (c * 255).astype(np.uint8), f)
    (tmp_path / "notes.txt").write_text("not a scan")
    found = scans.mesh_only_scans(str(tmp_path))
    assert [scans.mesh_only_scan_path(p) for p in found] == [
        ("40753679", str(tmp_path / "40753679.ply")),
        ("41069021", str(tmp_path / "41069021" / "41069021_3dod_mesh.ply"))]
    rv, rc, rf = scans.read_ply_mesh(scans.mesh_only_scan_path(found[1])[1])
    assert np.array_equal(rv, v) and np.array_equal(rf, f)


def test_points_table_and_refusals(tmp_path):
    from unscene3d_amd.datasets import preprocessing as P
    rng = np.random.default_rng(5)
    xyz, rgb = rng.random((7, 3)).astype(np.float32), rng.integers(0, 256, (7, 3)).astype(np.float64)
    normals, seg = rng.normal(size=(7, 3)).astype(np.float32), rng.integers(0, 900, 7)
    t = P.mesh_only_points_table(xyz, rgb, normals, seg)
    # arkit_preprocessing.py:102-116: coords | colours, normals | segment id | label, instance
    features = np.hstack((rgb, normals.astype(np.float64)))
    points = np.hstack((xyz.astype(np.float64), features))
    points = np.hstack((points, seg[..., None]))
    points = np.hstack((points, np.hstack((np.zeros((7, 1)), np.full((7, 1), -1.0)))))
    assert t.dtype == np.float32 and t.shape == (7, 12) and np.array_equal(t, points.astype(np.float32))
    with pytest.raises(ValueError, match="layout"):
        P.build_dataset(tmp_path, {"train": []}, tmp_path, tmp_path / "o", device="cpu", layout="s3dis")
    with pytest.raises(ValueError, match="ground truth"):
        P.build_dataset(tmp_path, {"train": []}, tmp_path, tmp_path / "o", device="cpu", layout="arkit", oracle=True)
    # a scan without pseudo-mask files is skipped before anything is read
    assert P.build_dataset(tmp_path, {"train": ["40753679"]}, tmp_path, tmp_path / "o", device="cpu",
                           layout="arkit") == {"train": []}
