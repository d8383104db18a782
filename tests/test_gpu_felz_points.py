"""GPU: the point-cloud over-segmentation (csrc/felz_points.hip, felzenszwalb_cpp.segment_points, layout="points")
against tests/felz_points_ref.py: edges as exact integers in order, weights bit for bit, partitions after
first-occurrence renumbering, and the layout through the scan builder and the tools."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import felz_points_ref as R
import test_gpu_scene_files_3d as S3
from normals_ref import knn_hybrid_f64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ------------------------------------------------------------------------------------------------- edges and weights
def _line():
    return np.array([[0, 0, 0], [1, 0, 0], [1.1, 0, 0]], F), 2, 5.0


EDGE_CASES = {
    "one_point": lambda: (np.array([[0.3, 0.2, 0.1]], F), 9, 1.0),
    "line_non_mutual": _line,
    "coincident": lambda: (R.coincident_four()[0], 3, 1.0),
    "k_plus_1_is_1": lambda: (_line()[0], 1, 5.0),
    "all_mutual_60": lambda: (np.random.default_rng(1).random((60, 3)).astype(F), 64, 10.0),
    "random_2047": lambda: (R.random_cloud(2047, 2047)[0], 9, R.RANDOM_RADIUS),
    "random_2048": lambda: (R.random_cloud(2048, 2048)[0], 9, R.RANDOM_RADIUS),
    "random_2049": lambda: (R.random_cloud(2049, 2049)[0], 9, R.RANDOM_RADIUS),
}


@pytest.fixture(scope="module", params=list(EDGE_CASES))
def edge_case(request, device):
    """One k-NN table on the device, its edges from the kernel and from the reference — computed once per case."""
    from unscene3d_amd import felzenszwalb_cpp as felz
    from unscene3d_amd import ops

    name = request.param
    points, k1, radius = EDGE_CASES[name]()
    n = points.shape[0]
    if name == "coincident":
        colors, normals = R.coincident_four()[1:]
    else:
        _, colors, normals = R.random_cloud(max(n, 25), 1000 + n)
        colors, normals = colors[:n], normals[:n]
    p = _dev(points, device)
    idx, count = ops.knn_hybrid(p, p, k1, radius)
    ref_idx, ref_count = knn_hybrid_f64(points, points, k1, radius)
    assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(count.cpu().numpy(), ref_count)
    ea, eb = felz.knn_edges(idx, count)
    ra, rb = R.knn_edges_ref(ref_idx, ref_count)
    return SimpleNamespace(name=name, points=points, colors=colors, normals=normals, idx=idx, count=count, ea=ea, eb=eb,
                           ra=ra, rb=rb, k1=k1)


def test_edges_equal_the_reference(edge_case):
    c = edge_case
    ea, eb = c.ea.cpu().numpy(), c.eb.cpu().numpy()
    assert ea.dtype == np.int32 and eb.dtype == np.int32
    assert np.array_equal(ea, c.ra) and np.array_equal(eb, c.rb)            # integers, order included
    expected = {"one_point": [], "line_non_mutual": [(0, 1), (1, 2)], "k_plus_1_is_1": [],
                "coincident": [(0, 1), (0, 3), (1, 3), (2, 0), (2, 1)]}
    if c.name in expected:
        assert list(zip(ea.tolist(), eb.tolist())) == expected[c.name]
    if c.name == "all_mutual_60":
        assert ea.size == 1770 and (ea < eb).all()
        assert (c.count.cpu().numpy() == 60).all() and (c.idx.cpu().numpy()[:, 60:] == -1).all()
    if c.name.startswith("random"):
        count = c.count.cpu().numpy()
        assert (count == 1).any() and (count < c.k1).sum() > 1000 and (count == c.k1).any() and (ea > eb).any()


def test_weights_equal_the_reference_bit_for_bit(edge_case, device):
    from unscene3d_amd import felzenszwalb_cpp as felz

    c = edge_case
    p, col, nor = (_dev(x, device) for x in (c.points, c.colors, c.normals))
    for oriented in (True, False):
        w = felz.point_edge_weights(p, col, nor, c.ea, c.eb, oriented=oriented).cpu().numpy()
        ref = R.edge_weights_ref(c.points, c.colors, c.normals, c.ra, c.rb, oriented)
        assert w.shape == ref.shape and np.isfinite(w).all()
        assert np.array_equal(_bits(w), _bits(ref)), (c.name, oriented)
    if c.name.startswith("random") or c.name == "coincident":
        assert (c.points[c.ra] == c.points[c.rb]).all(1).any()              # zero-length edges were among them


def test_oriented_weights_equal_the_mesh_kernel(device):
    """The mesh kernel's own (edge_a, edge_b, normals), fed to the point kernel: the same bits."""
    from unscene3d_amd import felzenszwalb_cpp as felz

    rng = np.random.default_rng(4)
    vertices, faces = S3._patch((0, 0, 0), (1.3, 0, 0), (0, 0.9, 0), 23, 17, 0)
    vertices = (vertices + rng.normal(0, 0.02, vertices.shape)).astype(F)       # rough: creases of both signs
    colors = (np.array([0.4, 0.5, 0.6]) + rng.uniform(-0.03, 0.03, vertices.shape)).astype(F)   # around the 0.05 threshold
    v, f, c = _dev(vertices, device), _dev(faces.astype(np.int32), device), _dev(colors, device)
    ea, eb, w, normals = felz.edge_weights(v, f, c)
    mine = felz.point_edge_weights(v, c, normals, ea, eb, oriented=True)
    assert ea.shape[0] == 3 * faces.shape[0] > 2000
    assert np.array_equal(_bits(mine.cpu().numpy()), _bits(w.cpu().numpy()))
    ref = R.edge_weights_ref(vertices, colors, normals.cpu().numpy(), ea.cpu().numpy(), eb.cpu().numpy(), True)
    assert np.array_equal(_bits(ref), _bits(w.cpu().numpy()))
    cd = np.abs(colors[ea.cpu().numpy()] - colors[eb.cpu().numpy()]).sum(1)
    assert 0.2 < (cd < 0.05).mean() < 0.8                                   # both branches of the squaring rule ran


def test_knn_edges_checks_a_callers_table(device):
    from unscene3d_amd import felzenszwalb_cpp as felz

    idx = torch.tensor([[0, 1], [1, 0], [2, 7]], dtype=torch.int32, device=device)
    count = torch.tensor([2, 2, 2], dtype=torch.int32, device=device)
    with pytest.raises(RuntimeError, match="outside"):
        felz.knn_edges(idx, count)
    count[2] = 1                                                             # the bad entry is past the row's count
    ea, eb = felz.knn_edges(idx, count)
    assert list(zip(ea.tolist(), eb.tolist())) == [(0, 1)]
    with pytest.raises(RuntimeError, match="outside"):
        felz.knn_edges(idx, torch.tensor([2, 2, 3], dtype=torch.int32, device=device))


# ------------------------------------------------------------------------------------------------------ segmentation
def _same_partition(labels, conn, ref_labels, ref_conn):
    got_labels, got_conn = R.renumbered(labels, conn)
    assert np.array_equal(got_labels, ref_labels)
    assert np.array_equal(got_conn, ref_conn)


def test_two_planes_with_given_normals(device):
    from unscene3d_amd import felzenszwalb_cpp as felz

    points, colors, normals, plane = R.two_planes()
    labels, conn = felz.segment_points(points, colors, normals, k=8, radius=0.12, kthr=0.005, segMinVerts=20, device=device)
    assert labels.dtype == np.int32 and conn.dtype == np.int32 and labels.shape == (800,)
    assert np.unique(labels).tolist() == [0, 1]                             # exactly two segments,
    assert all(np.unique(plane[labels == s]).size == 1 for s in (0, 1))     # each one plane only
    assert conn.tolist() == [[0, 1], [1, 0]]
    ref_labels, ref_conn, _ = R.segment_points_ref(points, colors, normals, True, **R.TWO_PLANES)
    _same_partition(labels, conn, ref_labels, ref_conn)
    # normals negated at random, weighted as unoriented: the same two segments
    flip = np.where(np.random.default_rng(5).random(800) < 0.5, -1, 1).astype(F)[:, None]
    sa, sb, sw = felz.point_graph(points, colors, normals * flip, 8, 0.12, device=device, oriented=False)
    again, again_conn = felz.relabel_symmetric(felz.merge_host(sa, sb, sw, 800, 0.005, 20), sa, sb)
    _same_partition(again, again_conn, ref_labels, ref_conn)
    ra, rb, rw = R.graph_ref(points, colors, normals * flip, False, 8, 0.12)
    assert np.array_equal(sa, ra) and np.array_equal(sb, rb) and np.array_equal(_bits(sw), _bits(rw))


@pytest.mark.parametrize("scene", ["two_planes", "random_2049"])
def test_estimated_normals(device, scene):
    """normals=None: the reference pipeline fed with the device's own estimate_normals output, weighted unoriented."""
    from unscene3d_amd import felzenszwalb_cpp as felz
    from unscene3d_amd import ops

    if scene == "two_planes":
        points, colors = R.two_planes()[:2]
        args = dict(R.TWO_PLANES)
    else:
        points, colors = R.random_cloud(2049, 2049)[:2]
        args = dict(k=8, radius=0.1, kthr=0.005, min_verts=20)
    labels, conn = felz.segment_points(points, colors, None, k=args["k"], radius=args["radius"], kthr=args["kthr"],
                                       segMinVerts=args["min_verts"], device=device)
    estimated = ops.estimate_normals(_dev(points, device)).cpu().numpy()
    ref_labels, ref_conn, _ = R.segment_points_ref(points, colors, estimated, False, **args)
    _same_partition(labels, conn, ref_labels, ref_conn)
    if scene == "two_planes":
        assert np.unique(labels).size == 2
    else:
        assert np.unique(labels).size > 3 and conn.shape[0] > 0
        assert np.array_equal(conn, np.unique(conn, axis=0)) and {tuple(p) for p in conn.tolist()} == {tuple(p[::-1]) for p in conn.tolist()}


def test_two_calls_give_the_same_bytes(device):
    from unscene3d_amd import felzenszwalb_cpp as felz
    from unscene3d_amd import ops

    points, colors, normals = R.random_cloud(2049, 2049)
    p, c, n = (_dev(x, device) for x in (points, colors, normals))
    runs = []
    for _ in range(2):
        idx, count = ops.knn_hybrid(p, p, 9, R.RANDOM_RADIUS)
        ea, eb = felz.knn_edges(idx, count)
        w1 = felz.point_edge_weights(p, c, n, ea, eb, True)
        w0 = felz.point_edge_weights(p, c, n, ea, eb, False)
        labels, conn = felz.segment_points(points, colors, normals, radius=R.RANDOM_RADIUS, device=device)
        runs.append([ea.cpu().numpy().tobytes(), eb.cpu().numpy().tobytes(), w1.cpu().numpy().tobytes(),
                     w0.cpu().numpy().tobytes(), labels.tobytes(), conn.tobytes()])
    assert runs[0] == runs[1]


# ---------------------------------------------------------------------------------------------------- small segments
@pytest.fixture(scope="module")
def cluster_scan(tmp_path_factory):
    root = tmp_path_factory.mktemp("cluster")
    points, colors, normals, plane = R.two_planes(cluster=True)
    rgb = np.rint(colors * 255).astype(np.uint8)
    R.write_ply_points(root / "room.ply", points, rgb, normals)
    return SimpleNamespace(path=str(root / "room.ply"), points=points, colors=(rgb / 255.0).astype(F), normals=normals,
                           plane=plane, rgb=rgb)


def test_small_segments(cluster_scan, device):
    from unscene3d_amd.pseudo_masks import scans

    s = cluster_scan
    args = dict(segments_min_verts=(20,), graph_k=8, graph_radius=0.12, device=device)
    ref_labels, ref_conn, _ = R.segment_points_ref(s.points, s.colors, s.normals, True, **R.TWO_PLANES)
    assert np.unique(ref_labels).size == 3

    keep = scans.load_point_cloud_scan(s.path, small_segments="keep", **args)
    assert keep["scene"] == "room" and keep["normals_from_file"] and np.array_equal(keep["normals"], s.normals)
    assert np.array_equal(keep["kept"], np.arange(805)) and keep["segments"].shape == (805, 1)
    _same_partition(keep["segment_ids"], keep["seg_connectivity"], ref_labels, ref_conn)
    third = keep["segment_ids"][-1]
    assert np.unique(keep["segment_ids"]).size == 3 and (keep["segment_ids"][-5:] == third).all()
    assert not np.isin(third, keep["seg_connectivity"])
    xyz = s.points.astype(np.float64)
    assert np.array_equal(keep["xyz"], xyz - xyz.min(0)) and np.array_equal(keep["rgb"], s.rgb.astype(np.float64))

    merge = scans.load_point_cloud_scan(s.path, small_segments="merge", **args)
    merged_ref = R.first_occurrence(R.merge_floaters_ref(ref_labels, ref_conn, 20, s.points))
    _same_partition(merge["segment_ids"], merge["seg_connectivity"], merged_ref,
                    R.symmetric_connectivity(merged_ref, *R.graph_ref(s.points, s.colors, s.normals, True, 8, 0.12)[:2]))
    ids = merge["segment_ids"]
    d = np.linalg.norm(s.points[:800].astype(np.float64) - s.points[800].astype(np.float64), axis=1)
    assert np.unique(ids).tolist() == [0, 1] and (ids[-5:] == ids[int(d.argmin())]).all()     # the nearest plane's label
    assert np.array_equal(np.unique(merge["seg_connectivity"]), [0, 1])                        # no third segment named
    assert np.array_equal(merge["kept"], np.arange(805))

    drop = scans.load_point_cloud_scan(s.path, small_segments="drop", **args)
    assert np.array_equal(drop["kept"], np.arange(800)) and drop["xyz"].shape == (800, 3)
    assert np.array_equal(drop["segment_ids"], keep["segment_ids"][:800]) and np.array_equal(drop["normals"], s.normals[:800])
    assert np.isin(drop["seg_connectivity"], drop["segment_ids"]).all() and drop["seg_connectivity"].shape == (2, 2)


def test_levels_share_one_graph(cluster_scan, device):
    from unscene3d_amd import felzenszwalb_cpp as felz
    from unscene3d_amd.pseudo_masks import scans

    s = cluster_scan
    m = scans.load_point_cloud_scan(s.path, (3, 20, 500), 1, graph_k=8, graph_radius=0.12, small_segments="keep", device=device)
    assert m["segments"].shape == (805, 3) and np.array_equal(m["segment_ids"], m["segments"][:, 1])
    for level, least in enumerate((3, 20, 500)):
        labels, _ = felz.segment_points(s.points, s.colors, s.normals, 8, 0.12, 0.005, least, device=device)
        assert np.array_equal(m["segments"][:, level], labels)
    assert [np.unique(m["segments"][:, level]).size for level in range(3)] == [3, 3, 2]      # 500: the planes join


# ------------------------------------------------------------------------------------------------------------ layout
VOXEL, LEVELS, GRAPH = 0.06, (20, 40), ("--graph-k", "8", "--graph-radius", "0.15")
DIR_SCENE, FLAT_SCENE = "office_1", "hallway_2"
OFFSET = np.array([1.5, -2.0, 0.25])


def _scan_cloud(seed, with_normals):
    """The 2590 vertices of the floor-and-two-boxes mesh as a cloud (no faces), jittered; one colour per patch (they
    differ by 0.15 or more between touching patches, shaded by position inside a patch) and the patches' normals."""
    rng = np.random.default_rng(seed)
    vertices = S3._mesh()[0]
    points = (vertices + rng.normal(0, 0.004, vertices.shape) + OFFSET).astype(F)
    patch = np.concatenate([np.zeros(900, np.int64), np.repeat(np.arange(1, 11), 169)])
    palette = (np.array([[3, 1, 2], [0, 4, 1], [5, 2, 0], [1, 0, 5], [4, 5, 3], [2, 3, 4]]) * 40 + 20)[np.arange(11) % 6]
    rgb = ((palette[patch] + np.floor(vertices * 4) + seed) % 256).astype(np.uint8)
    sides = [(0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)]
    normals = np.concatenate([np.tile((0, 0, 1), (900, 1))] + [np.tile(n, (169, 1)) for _ in range(2) for n in sides])
    return points, rgb, normals.astype(F) if with_normals else None, patch


@pytest.fixture(scope="module")
def scans_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("points_layout")
    os.makedirs(root / "scans" / DIR_SCENE)
    clouds = {DIR_SCENE: _scan_cloud(0, True), FLAT_SCENE: _scan_cloud(40, False)}
    R.write_ply_points(root / "scans" / DIR_SCENE / f"{DIR_SCENE}.ply", *clouds[DIR_SCENE][:3])
    R.write_ply_points(root / "scans" / f"{FLAT_SCENE}.ply", *clouds[FLAT_SCENE][:3], fmt="ascii")
    return SimpleNamespace(root=root, scans=str(root / "scans"), clouds=clouds)


def _expected_xyz(cloud):
    xyz = cloud[0].astype(np.float64)
    return (xyz - xyz.min(0)).astype(F)


def test_build_scene(scans_root, device):
    from unscene3d_amd import felzenszwalb_cpp as felz
    from unscene3d_amd.models.weights import load_csc_backbone
    from unscene3d_amd.pseudo_masks import scans

    torch.manual_seed(0)
    model_3d = load_csc_backbone({}, device=device)
    cloud = scans_root.clouds[DIR_SCENE]
    scan = os.path.join(scans_root.scans, DIR_SCENE)
    s = scans.build_scene(scan, None, voxel_size=VOXEL, segments_min_verts=LEVELS, device=device, model_3d=model_3d,
                          layout="points", graph_radius=0.15, small_segments="keep")
    assert set(s) == {"coords", "colors", "feats_3d", "resolution_scale", "segment_ids", "seg_connectivity",
                      "full_res_coords", "voxel_size"}                       # geometry only
    n, full = s["coords"].shape[0], s["full_res_coords"]
    assert full.dtype == F and np.array_equal(full, _expected_xyz(cloud)) and (full.min(0) == 0).all()
    assert s["coords"].dtype == np.int32 and s["coords"].shape == (n, 4) and 1000 < n <= 2590
    assert s["feats_3d"].shape == (n, 96) and np.isfinite(s["feats_3d"]).all()
    assert s["segment_ids"].dtype == np.int64 and s["segment_ids"].shape == (n,)
    labels, conn = felz.segment_points(cloud[0], (cloud[1] / 255.0).astype(F), cloud[2], 8, 0.15, 0.005, LEVELS[0],
                                       device=device)
    m = scans.load_point_cloud_scan(scan, LEVELS, 0, graph_radius=0.15, small_segments="keep", device=device)
    assert np.array_equal(m["segment_ids"], labels) and np.array_equal(m["seg_connectivity"], conn)
    # segment_ids[kept]: the scene file holds the segment of each voxel's first point
    from unscene3d_amd import MinkowskiEngine as ME
    grid = np.floor(m["xyz"] * (1.0 / VOXEL)).astype(np.int32)
    kept = ME.utils.sparse_quantize(grid, return_index=True, device=device)[1].cpu().numpy()
    assert np.array_equal(s["segment_ids"], labels[kept].astype(np.int64))
    assert np.array_equal(s["seg_connectivity"], conn.astype(np.int64))
    # inside a patch the given normals are equal, so every weight there is exactly 0; between patches the normals are
    # orthogonal and the colours 0.15 or more apart, far above kthr: the segments are the 11 patches
    assert np.array_equal(R.first_occurrence(labels), cloud[3])
    other = scans.build_scene(scan, None, voxel_size=VOXEL, segments_min_verts=LEVELS, device=device, model_3d=model_3d,
                              layout="points", graph_radius=0.15, small_segments="keep", segment_dimension_order=1)
    assert np.unique(other["segment_ids"]).size <= np.unique(s["segment_ids"]).size
    flat = scans.build_scene(os.path.join(scans_root.scans, FLAT_SCENE + ".ply"), None, voxel_size=VOXEL,
                             segments_min_verts=LEVELS, device=device, model_3d=model_3d, layout="points", graph_radius=0.15)
    assert np.array_equal(flat["full_res_coords"], _expected_xyz(scans_root.clouds[FLAT_SCENE]))
    with pytest.raises(ValueError, match="layout"):
        scans.build_scene(scan, None, model_3d=model_3d, layout="s3dis")


def _run(tool, *argv):
    """A tool of the repository in a fresh child process under its own time limit -> CompletedProcess."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), *argv], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=300)


def test_tools_end_to_end(scans_root, device):
    """scene_files_from_scans.py, pseudo_masks_run.py and dataset_from_scans.py --write-connectivity on two scans."""
    import yaml

    from unscene3d_amd import ops
    from unscene3d_amd.pseudo_masks import scans

    root, levels = scans_root.root, [str(n) for n in LEVELS]
    scenes, masks, data = str(root / "scenes"), str(root / "masks"), str(root / "data")
    r = _run("scene_files_from_scans.py", "--scans", scans_root.scans, "--out", scenes, "--layout", "points", *GRAPH,
             "--csc-random-weights", "0", "--voxel-size", str(VOXEL), "--segments-min-verts", *levels)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(scenes)) == [FLAT_SCENE + ".npz", DIR_SCENE + ".npz"]
    r = _run("pseudo_masks_run.py", "--scenes", scenes, "--out", masks)
    assert r.returncode == 0, r.stderr[-2000:]
    r = _run("dataset_from_scans.py", "--scans", scans_root.scans, "--pseudo", masks, "--out", data, "--layout", "points",
             *GRAPH, "--segments-min-verts", *levels, "--write-connectivity")
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["scans"] == {"train": 2}
    with open(os.path.join(data, "train_database.yaml")) as f:
        entries = yaml.safe_load(f)
    assert [e["scene"] for e in entries] == [FLAT_SCENE, DIR_SCENE]
    assert not os.path.exists(os.path.join(data, "instance_gt"))
    for e in entries:
        scene = e["scene"]
        cloud = scans_root.clouds[scene]
        points = np.load(e["filepath"])
        assert e["scene_type"] == "room" and e["file_len"] == 2590 and e["segments_min_verts"] == LEVELS[0]
        assert points.dtype == F and points.shape == (2590, 12)
        assert np.array_equal(points[:, :3], _expected_xyz(cloud))
        assert np.array_equal(points[:, :3], np.load(os.path.join(masks, f"{scene}_cloud.npy")))
        assert np.array_equal(points[:, 3:6], cloud[1].astype(F))
        if cloud[2] is not None:                                            # the file's normals, else estimated ones
            assert np.array_equal(_bits(points[:, 6:9]), _bits(cloud[2]))
        else:
            est = ops.estimate_normals(_dev(points[:, :3], device), 0.1, 30)
            assert np.array_equal(_bits(points[:, 6:9]), _bits(est.cpu().numpy()))
        m = scans.load_point_cloud_scan(e["raw_filepath"], LEVELS, 0, graph_k=8, graph_radius=0.15, device=device)
        assert m["normals_from_file"] == (cloud[2] is not None)
        assert np.array_equal(points[:, 9], m["segment_ids"].astype(F))
        assert not points[:, 10].any() and (points[:, 11] == -1).all()
        conn = np.load(e["connectivity_filepath"])
        assert conn.dtype == np.int32 and np.array_equal(conn, m["seg_connectivity"]) and conn.shape[0] > 0
        freemasks = np.load(e["freemask_filepath"])
        assert freemasks.shape[0] == 2590 and freemasks.shape[1] > 0
