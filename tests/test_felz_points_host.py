"""CPU: the numpy restatement of the point-cloud over-segmentation (tests/felz_points_ref.py) on answers known by hand,
`scans.read_ply_points`, `scans.merge_floaters`, and the argument refusals that come before any device work."""
import numpy as np
import pytest

import felz_points_ref as R
from knn_ref import knn1_f64
from normals_ref import knn_hybrid_f64

F = np.float32


# ------------------------------------------------------------------------------------------------- the ref's answers
def test_edge_rule_known_answers():
    line = np.array([[0, 0, 0], [1, 0, 0], [1.1, 0, 0]], F)
    idx, count = knn_hybrid_f64(line, line, 2, 5.0)
    assert idx.tolist() == [[0, 1], [1, 2], [2, 1]]                 # 0 is not in 1's list: the non-mutual case
    a, b = R.knn_edges_ref(idx, count)
    assert list(zip(a.tolist(), b.tolist())) == [(0, 1), (1, 2)]
    a, b = R.knn_edges_ref(np.array([[0]], np.int32), np.array([1], np.int32))
    assert a.size == 0 and b.size == 0 and a.dtype == np.int32      # one point; also k + 1 = 1
    idx, count = knn_hybrid_f64(line, line, 1, 5.0)
    assert R.knn_edges_ref(idx, count)[0].size == 0
    points = R.coincident_four()[0]
    idx, count = knn_hybrid_f64(points, points, 3, 1.0)
    assert idx.tolist() == [[0, 1, 3], [0, 1, 3], [2, 0, 1], [0, 1, 3]]      # row 3 lists itself last
    a, b = R.knn_edges_ref(idx, count)
    assert list(zip(a.tolist(), b.tolist())) == [(0, 1), (0, 3), (1, 3), (2, 0), (2, 1)]
    cloud = np.random.default_rng(1).random((60, 3)).astype(F)
    idx, count = knn_hybrid_f64(cloud, cloud, 64, 10.0)
    assert (count == 60).all() and (idx[:, 60:] == -1).all()
    a, b = R.knn_edges_ref(idx, count)
    assert a.size == 1770 and (a < b).all() and len(set(zip(a.tolist(), b.tolist()))) == 1770


def test_a_reversed_row_order_changes_nothing_but_the_direction():
    """Every undirected pair of either list exactly once, whichever row emits it."""
    points = R.random_cloud(300, 3)[0]
    idx, count = knn_hybrid_f64(points, points, 5, 0.2)
    a, b = R.knn_edges_ref(idx, count)
    pairs = {(min(i, int(j)), max(i, int(j))) for i in range(300) for j in idx[i, :count[i]] if j != i}
    assert len(a) == len(pairs) and {(min(x, y), max(x, y)) for x, y in zip(a.tolist(), b.tolist())} == pairs
    assert (a > b).any()                                            # some pairs are not mutual


def test_weight_known_answers():
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0]], F)
    C = np.array([[0.5, 0.5, 0.5], [0.5, 0.52, 0.51], [0.8, 0.2, 0.2]], F)
    N = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 0, -1]], F)
    a, b = np.array([0, 1, 0, 0], np.int32), np.array([1, 0, 2, 1], np.int32)
    w1 = R.edge_weights_ref(P, C, N, a, b, True)
    base = (1 - 0.8) * 0.03
    # 0 -> 1: the far normal (0.6, 0, 0.8) leans along +x: squared.  1 -> 0: the far normal is +z, the edge -x: not.
    assert w1.dtype == F and np.allclose(w1[[0, 1, 3]], [base * base, base, base * base], rtol=1e-5)
    assert np.isfinite(w1[2]) and np.isclose(w1[2], 2.0 * 0.9, rtol=1e-6)    # coincident, opposite normals: (1 + 1) * 0.9
    w0 = R.edge_weights_ref(P, C, N, a, b, False)
    assert np.allclose(w0[[0, 1, 3]], base, rtol=1e-5) and w0[2] == 0        # |dot| = 1: no distance, nothing squared
    flipped = N * np.array([[1], [-1], [1]], F)
    assert np.array_equal(R.edge_weights_ref(P, C, flipped, a, b, False).view(np.uint32), w0.view(np.uint32))
    assert not np.array_equal(R.edge_weights_ref(P, C, flipped, a, b, True), w1)


def test_weights_round_every_operation_in_float32():
    points, colors, normals = R.random_cloud(500, 9)
    idx, count = knn_hybrid_f64(points, points, 6, 0.2)
    a, b = R.knn_edges_ref(idx, count)
    for oriented in (True, False):
        w = R.edge_weights_ref(points, colors, normals, a, b, oriented)
        exact = R.edge_weights_ref(*(x.astype(np.float64).astype(F) for x in (points, colors, normals)), a, b, oriented)
        assert np.array_equal(w, exact) and np.isfinite(w).all()
        P, C, N = (x.astype(np.float64) for x in (points, colors, normals))
        dot = (N[a] * N[b]).sum(1)
        cd = np.abs(C[a] - C[b]).sum(1)
        f64 = (1 - (dot if oriented else np.abs(dot))) * cd
        if oriented:
            d = P[b] - P[a]
            with np.errstate(invalid="ignore"):
                along = (N[b] * d).sum(1) / np.linalg.norm(d, axis=1)
            f64 = np.where((along > 0) & (cd < 0.05), f64 * f64, f64)
        sure = np.abs(cd - 0.05) > 1e-6                            # a colour distance on the threshold may fall either way
        assert sure.sum() > len(a) - 5 and np.allclose(w[sure], f64[sure], rtol=1e-4, atol=1e-7)


def test_merge_known_answers():
    a, b = np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 3, 4], np.int32)
    w = np.array([0.0, 0.001, 0.004, 1.0], F)
    # 0-1 joins (0 <= 0.005), limit 0 + 0.005/2; 1-2 joins (0.001 <= 0.0025), limit 0.001 + 0.005/3 = 0.00267;
    # 2-3 does not (0.004 > 0.00267); 3-4 does not.
    assert R.first_occurrence(R.merge_ref(a, b, w, 5, 0.005, 1)).tolist() == [0, 0, 0, 1, 2]
    assert R.first_occurrence(R.merge_ref(a, b, w, 5, 0.005, 2)).tolist() == [0, 0, 0, 0, 0]     # 3 joins {0,1,2}; then 4
    assert R.first_occurrence(R.merge_ref(a, b, w, 5, 0.01, 1)).tolist() == [0, 0, 0, 0, 1]      # 0.004 <= 0.001 + 0.01/3
    assert R.first_occurrence([7, 7, 2, 9, 2]).tolist() == [0, 0, 1, 2, 1]
    labels, conn = R.renumbered(np.array([5, 5, 1, 3]), np.array([[1, 5], [5, 1], [3, 1], [1, 3]]))
    assert labels.tolist() == [0, 0, 1, 2] and conn.tolist() == [[0, 1], [1, 0], [1, 2], [2, 1]]


def test_two_planes_reference_gives_two_pure_segments():
    points, colors, normals, plane = R.two_planes()
    labels, conn, (a, b, w) = R.segment_points_ref(points, colors, normals, True, **R.TWO_PLANES)
    cross = plane[a] != plane[b]
    assert 3000 < len(a) < 3600 and 50 < cross.sum() < 150
    assert (w[~cross] == 0).all() and (w[cross] >= F(1.2)).all()
    assert np.unique(labels).size == 2 and all(np.unique(plane[labels == s]).size == 1 for s in (0, 1))
    assert conn.tolist() == [[0, 1], [1, 0]]
    flip = np.where(np.random.default_rng(5).random(800) < 0.5, -1, 1).astype(F)[:, None]
    unoriented, _, _ = R.segment_points_ref(points, colors, normals * flip, False, **R.TWO_PLANES)
    assert np.array_equal(unoriented, labels)


# --------------------------------------------------------------------------------------------------- package, no GPU
def test_merge_floaters_matches_the_reference():
    from unscene3d_amd.pseudo_masks import scans

    points, colors, normals, plane = R.two_planes(cluster=True)
    labels, conn, _ = R.segment_points_ref(points, colors, normals, True, **R.TWO_PLANES)
    assert np.unique(labels).size == 3 and (labels[-5:] == 2).all() and not np.isin(2, conn)
    nearest = lambda q, r: knn1_f64(points[q], points[r])[0]
    merged = scans.merge_floaters(labels, conn, 20, nearest)
    assert np.array_equal(merged, R.merge_floaters_ref(labels, conn, 20, points))
    assert np.unique(merged).size == 2 and (merged[-5:] == labels[plane == 0][0]).all()     # the floor is nearer
    assert np.array_equal(merged[:-5], labels[:-5])
    assert np.array_equal(scans.merge_floaters(labels, conn, 401, nearest), np.zeros(805, np.int64))    # nothing kept
    assert np.array_equal(scans.merge_floaters(labels[:-5], conn, 20, nearest), labels[:-5])          # no floater
    # a segment of full size that no pair names is a floater too
    far = np.where(np.arange(805) >= 800, 2, labels)
    big = scans.merge_floaters(far, conn, 3, nearest)
    assert np.array_equal(big, R.merge_floaters_ref(far, conn, 3, points)) and np.unique(big).size == 2


@pytest.mark.parametrize("fmt", ["binary_little_endian", "ascii"])
@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_faces", [False, True])
def test_read_ply_points(tmp_path, fmt, with_normals, with_faces):
    from unscene3d_amd.pseudo_masks import scans

    rng = np.random.default_rng(2)
    points = rng.normal(size=(37, 3)).astype(F)
    rgb = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    normals = rng.normal(size=(37, 3)).astype(F) if with_normals else None
    faces = rng.integers(0, 37, (11, 3)) if with_faces else None
    path = tmp_path / "cloud.ply"
    R.write_ply_points(path, points, rgb, normals, faces, fmt)
    p, c, n = scans.read_ply_points(path)
    assert p.dtype == F and np.array_equal(p, points)
    assert c.dtype == F and np.array_equal(c, (rgb / 255.0).astype(F))
    assert (n is None) if not with_normals else (n.dtype == F and np.array_equal(n, normals))
    if with_faces:                                                  # the same file is a mesh to the mesh reader
        assert np.array_equal(scans.read_ply_mesh(path)[2], faces)
    else:
        with pytest.raises(ValueError, match="face"):
            scans.read_ply_mesh(path)


def test_read_ply_points_refuses_a_file_without_colours(tmp_path):
    from unscene3d_amd.pseudo_masks import scans

    path = tmp_path / "bare.ply"
    path.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                     b"end_header\n0 0 0\n")
    with pytest.raises(ValueError, match="red"):
        scans.read_ply_points(path)


def test_scan_paths(tmp_path):
    from unscene3d_amd.pseudo_masks import scans

    (tmp_path / "room_a").mkdir()
    (tmp_path / "room_b.ply").write_bytes(b"")
    assert scans.point_cloud_scan_path(tmp_path / "room_a") == ("room_a", str(tmp_path / "room_a" / "room_a.ply"))
    assert scans.point_cloud_scan_path(tmp_path / "room_b.ply") == ("room_b", str(tmp_path / "room_b.ply"))
    assert scans.point_cloud_scan_path(tmp_path / "room_b") == ("room_b", str(tmp_path / "room_b.ply"))
    assert scans.point_cloud_scans(tmp_path) == [str(tmp_path / "room_a"), str(tmp_path / "room_b.ply")]


def test_refusals_come_before_any_device_work(tmp_path):
    """Each of these raises ValueError from the arguments alone: nothing is read, no device is asked for."""
    from unscene3d_amd import felzenszwalb_cpp as felz
    from unscene3d_amd.datasets import preprocessing as P
    from unscene3d_amd.pseudo_masks import scans

    points, colors, normals, _ = R.two_planes()
    with pytest.raises(ValueError, match="k must be"):
        felz.segment_points(points, colors, normals, k=64)
    with pytest.raises(ValueError, match="k must be"):
        felz.segment_points(points, colors, normals, k=-1)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            felz.segment_points(points, colors, normals, radius=radius)
    with pytest.raises(ValueError, match="colors"):
        felz.segment_points(points, colors[:-1], normals)
    with pytest.raises(ValueError, match="normals"):
        felz.segment_points(points, colors, normals[:, :2])
    with pytest.raises(ValueError, match="points"):
        felz.segment_points(points[:0], colors[:0])
    missing = tmp_path / "no_such_scan"
    with pytest.raises(ValueError, match="small_segments"):
        scans.load_point_cloud_scan(missing, small_segments="absorb")
    with pytest.raises(ValueError, match="segment_dimension_order"):
        scans.load_point_cloud_scan(missing, (20, 50), segment_dimension_order=2)
    with pytest.raises(ValueError, match="graph_k"):
        scans.load_point_cloud_scan(missing, graph_k=64)
    with pytest.raises(ValueError, match="graph_radius"):
        scans.load_point_cloud_scan(missing, graph_radius=0)
    with pytest.raises(ValueError, match="model_3d"):
        scans.build_scene(missing, None, layout="points")
    for build in (lambda: scans.build_scene(missing, None, model_3d=object(), layout="s3dis"),
                  lambda: P.build_dataset(missing, {}, None, tmp_path / "out", layout="s3dis")):
        with pytest.raises(ValueError, match="'scannet', 'arkit' or 'points'"):
            build()
    with pytest.raises(ValueError, match="ground truth"):
        P.build_dataset(missing, {}, None, tmp_path / "out", layout="points", oracle=True)
    assert not (tmp_path / "out").exists()
