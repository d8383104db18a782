"""Scan directories + pseudo-mask files -> the dataset `FreeMaskSceneReader` trains on (reference
datasets/preprocessing/freemask_preprocessing.py: `process_file` :66-220, `compute_color_mean_std` :222-240,
`create_label_database` :55-64, base_preprocessing.py `save_database`).

A scan directory `SCANS/scene0000_00/` holds ScanNet's files:

    scene0000_00.txt                          `key = value` lines; axisAlignment is used
    scene0000_00_vh_clean_2.ply               the coloured mesh
    scene0000_00_vh_clean_2.labels.ply        optional: the `label` vertex property (ground truth)
    *[0-9].segs.json                          optional: segIndices, one per vertex
    *.aggregation.json                        optional: segGroups (instance id + segments)

and `PSEUDO/scene0000_00_cloud.npy` / `_masks.npy` are what tools/pseudo_masks_run.py wrote for it.  `build_dataset`
writes, under OUT:

    {mode}/0000_00.npy               f32[N,12]: xyz (raw, not aligned), rgb 0..255, normal, segment id, label, instance
    {mode}/0000_00_freemasks.npy     f32[N,K]: the pseudo masks lifted to the mesh vertices
    instance_gt/{mode}/scene0000_00.txt      label * 1000 + instance + 1 per vertex (only with ground-truth files)
    {mode}_database.yaml, label_database.yaml, color_mean_std.yaml

The readers are numpy only (pseudo_masks/scans.py); the reference reads the same files through open3d and plyfile.
Device work: the vertex normals (`ops.mesh_vertex_normals`), the 1-NN lift of the masks (`ops.knn1` + a row gather),
the over-segmentation when no segs.json exists.

Deviations from the reference: normals stored in the PLY are not read (ScanNet's meshes have none; the reference
computes them in that case, as here); the 1-NN search runs on f32 coordinates (the reference's KDTree on f64); a scan
without ground-truth files is processed (label 0, instance -1), where the reference fails on the missing files;
`color_mean_std.yaml` comes from the train database when one is written, else from the validation database (the
reference's driver always passes the validation database, base_preprocessing.py:55-57).  Not built: the
S3DIS layout, chunked scenes.

Mesh-only scans (`layout="arkit"`; reference datasets/preprocessing/arkit_preprocessing.py `process_file`): a scan is
`SCANS/{scene}/{scene}_3dod_mesh.ply` or `SCANS/{scene}.ply`, and `build_dataset` writes `{mode}/{scene}.npy`,
`{mode}/{scene}_freemasks.npy` and database entries with the reference's placeholders (`scene_type: room`, empty raw
description / instance / segmentation paths).  The normal columns are ESTIMATED FROM THE POINTS,
`ops.estimate_normals(xyz, 0.1, 30)` (:98-101: open3d's estimate_normals with KDTreeSearchParamHybrid(0.1, 30)), since
these meshes carry no usable normals at that stage.
Deviation: the published reader indexes a 9-column cloud file (`cloud_np[:, 3:6]`, `[:, 7]`, `[:, 8]`, `[:, -1]`,
:90-95), but its own pseudo-mask writer produces such a file only in a commented-out branch — whose columns disagree
with those indices by one — and the live writer saves xyz only, as tools/pseudo_masks_run.py does.  So colours and
segment ids come from the mesh: the builder re-runs the scan builder's deterministic mesh stages
(`scans.load_mesh_only_scan`) and requires `{scene}_cloud.npy` to equal the kept, shifted vertices row for row, bit for
bit in f32 (ValueError naming the scene otherwise); the masks are then taken row for row, with no 1-NN.  There is no
ground truth: label 0, instance -1 and no `instance_gt` file, this builder's convention for scans without ground truth.

Point-cloud scans (`layout="points"`): `SCANS/{scene}/{scene}.ply` or `SCANS/{scene}.ply` with a vertex
element only.  The same files and entries as for a mesh-only scan, through `build_point_cloud_tables`: xyz, colours and
segment ids are `scans.load_point_cloud_scan`'s; the normal columns are the file's nx, ny, nz when it has them, else
`ops.estimate_normals(xyz, 0.1, 30)`.  Ground-truth columns (S3DIS's annotation folders) are not read."""
from __future__ import annotations

import glob
import json
import os
import re

import numpy as np
import torch

from .. import ops
from ..pseudo_masks import scans

# the ScanNet benchmark's 20 class ids without wall (1) and floor (2): freemask_preprocessing.py:19
FOREGROUND_CLASS_IDS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)
LABEL_DATABASE = {0: {"color": [0, 0, 0], "name": "background", "validation": True},
                  1: {"color": [0, 0, 128], "name": "foreground", "validation": True}}
SCENE_DIR = re.compile(r"scene(\d{4})_(\d{2})")


def parse_scene_dir(scan_dir):
    """`.../scene0123_01` -> (name, 123, 1).  The reader derives file and scene names from these numbers, so any other
    directory name raises ValueError."""
    name = os.path.basename(os.path.normpath(os.fspath(scan_dir)))
    m = SCENE_DIR.fullmatch(name)
    if m is None:
        raise ValueError(f"{scan_dir}: a scan directory must be named scene<4 digits>_<2 digits>")
    return name, int(m.group(1)), int(m.group(2))


def _first(pattern):
    found = sorted(glob.glob(pattern))
    return found[0] if found else None


def _read_json(path):
    with open(path) as f:
        return json.load(f)


def read_axis_alignment(info_path):
    """The axisAlignment line of `{scene}.txt` -> f64[4,4]; identity when the file has none (:174-181)."""
    with open(info_path) as f:
        for line in f:
            key, _, val = line.partition(" = ")
            if key.strip() == "axisAlignment":
                axis = np.array([float(t) for t in val.split()], np.float64)
                if axis.size != 16:
                    raise ValueError(f"{info_path}: axisAlignment has {axis.size} values, expected 16")
                return axis.reshape(4, 4)
    return np.identity(4)


def scene_labels(segments, labels, seg_groups, foreground_ids=FOREGROUND_CLASS_IDS):
    """freemask_preprocessing.py:130-144 as written -> int64[N,2] (label, instance).  `segments`: the raw segIndices;
    `labels`: the labels PLY's ids; `seg_groups`: aggregation.json's segGroups.  Every vertex of a group's segments gets
    the group's id (a later group overwrites an earlier one).  Labels in `foreground_ids` become 1; labels OUTSIDE the
    list KEEP THEIR ID (wall stays 1 — the same number as foreground — floor 2, and any other id as it is: the
    reference's quirk, kept because its ground-truth files were produced with it); instances of labels outside the
    list become -1."""
    out = np.stack([np.asarray(labels).astype(np.int64), np.full(len(labels), -1, np.int64)], 1)
    for group in seg_groups:
        out[np.isin(segments, np.array(group["segments"])), 1] = group["id"]
    foreground = np.isin(out[:, 0], foreground_ids)
    out[foreground, 0] = 1
    out[~foreground, 1] = -1
    return out


def lift_masks(aligned_xyz, cloud, masks, device="cuda"):
    """Rows of `masks` (bool or f32 [M,K]) at the nearest `cloud` point (f32/f64 [M,>=3]) of every aligned vertex ->
    f32[N,K] (freemask_preprocessing.py:209-217), search and gather on the device."""
    dev = torch.device(device)
    q = torch.as_tensor(np.ascontiguousarray(aligned_xyz, dtype=np.float32), device=dev)
    ref = torch.as_tensor(np.ascontiguousarray(np.asarray(cloud)[:, :3], dtype=np.float32), device=dev)
    m = np.asarray(masks)
    if m.ndim != 2 or m.shape[0] != ref.shape[0]:
        raise ValueError(f"pseudo masks {list(m.shape)} do not match the cloud's {ref.shape[0]} points")
    _, ind = ops.knn1(q, ref)
    return torch.as_tensor(np.ascontiguousarray(m), device=dev)[ind].to(torch.float32).cpu().numpy()


def build_scene_tables(scan_dir, pseudo_dir, oracle=False, device="cuda", foreground_ids=FOREGROUND_CLASS_IDS,
                       segments_min_verts=20):
    """One scan -> dict(points f32[N,12], freemasks f32[N,K], gt int32[N] or None, color_mean, color_std (3 floats
    each), raw paths), or None (with a message) when the scan's pseudo-mask files are missing — `process_file`.

    points: xyz as stored, integer colours as stored, vertex normals, segment id (`np.unique(segIndices,
    return_inverse=True)` of segs.json, else `felzenszwalb_cpp.segment_mesh(..., 0.005, segments_min_verts)`,
    conf/data/indoor.yaml:47), label, instance (`scene_labels`; without ground-truth files 0 and -1).
    gt = label * 1000 + instance + 1.  color_mean / color_std: mean of c / 255 and of (c / 255)^2 per channel in f64
    (:162-171; "std" is the second moment, `color_mean_std` turns it into a deviation).
    connectivity: int32[P,2], the over-segmentation's directed segment pairs, or None when the segment ids came from a
    segs.json (which carries no adjacency).
    freemasks: the pseudo masks at the nearest cloud point of every vertex aligned with axisAlignment; `oracle=True`:
    one column per ground-truth instance i in range(number of instance ids), set where instance == i (:188-192)."""
    from .. import felzenszwalb_cpp

    dev = torch.device(device)
    scene, _, _ = parse_scene_dir(scan_dir)
    scan_dir = os.fspath(scan_dir)
    mesh_path = os.path.join(scan_dir, f"{scene}_vh_clean_2.ply")
    info_path = os.path.join(scan_dir, f"{scene}.txt")
    cloud = masks = None
    if not oracle:                                    # before any device work: a scan without masks is skipped
        try:
            cloud = np.load(os.path.join(pseudo_dir, f"{scene}_cloud.npy"))
            masks = np.load(os.path.join(pseudo_dir, f"{scene}_masks.npy"))
        except FileNotFoundError as e:
            print(f"Could not load pseudo masks for {scene}: {e.filename}")
            return None

    vertices, colors01, faces = scans.read_ply_mesh(mesh_path)
    raw = scans.read_ply_vertex_properties(mesh_path, ("red", "green", "blue"))
    rgb = np.stack([raw[n] for n in ("red", "green", "blue")], 1).astype(np.uint8)      # load_ply: dtype=np.uint8
    v_d = torch.from_numpy(vertices).to(dev)
    f_d = torch.from_numpy(faces).to(dev)
    normals = ops.mesh_vertex_normals(v_d, f_d).cpu().numpy()
    features = np.hstack([rgb.astype(np.float64), normals.astype(np.float64)])

    seg_path = _first(os.path.join(glob.escape(scan_dir), "*[0-9].segs.json"))
    agg_path = _first(os.path.join(glob.escape(scan_dir), "*.aggregation.json"))
    label_path = mesh_path.replace(".ply", ".labels.ply")
    segments = connectivity = None
    if seg_path is not None:
        segments = np.array(_read_json(seg_path)["segIndices"])
        if segments.shape != (vertices.shape[0],):
            raise ValueError(f"{seg_path}: {segments.shape[0]} segIndices for {vertices.shape[0]} vertices")
        segment_ids = np.unique(segments, return_inverse=True)[1].reshape(-1)
    else:
        segment_ids, connectivity = felzenszwalb_cpp.segment_mesh(v_d, f_d, torch.from_numpy(colors01).to(dev), 0.005,
                                                                  int(segments_min_verts), device=dev)
    has_gt = agg_path is not None and os.path.exists(label_path)
    if has_gt:
        if segments is None:
            raise ValueError(f"{agg_path}: instance groups need the segIndices of a segs.json beside it")
        lab = scans.read_ply_vertex_properties(label_path, ("x", "y", "z", "label"))
        if not np.allclose(vertices, np.stack([lab["x"], lab["y"], lab["z"]], 1).astype(np.float32)):
            raise ValueError(f"{label_path}: files doesn't have same coordinates")
        labels = scene_labels(segments, lab["label"].astype(np.uint32), _read_json(agg_path)["segGroups"],
                              foreground_ids)
    else:
        labels = np.stack([np.zeros(vertices.shape[0], np.int64), np.full(vertices.shape[0], -1, np.int64)], 1)
    points = np.hstack([vertices, features, np.asarray(segment_ids, np.int64)[:, None], labels])     # f64, as :92-145
    gt = (points[:, -2] * 1000 + points[:, -1] + 1).astype(np.int32) if has_gt else None

    if oracle:
        n_inst = len(set(np.unique(labels[:, 1]).tolist()) - {-1})
        freemasks = np.zeros((points.shape[0], n_inst), np.float32)
        for i in range(n_inst):
            freemasks[labels[:, 1] == i, i] = 1.0
    else:
        axis = read_axis_alignment(info_path)
        homo = np.hstack([points[:, :3], np.ones((points.shape[0], 1))])
        freemasks = lift_masks(homo @ axis.T[:, :3], cloud, masks, device=dev)

    mean, second = color_moments(features[:, :3])
    return {"points": points.astype(np.float32), "freemasks": freemasks, "gt": gt, "color_mean": mean, "color_std": second,
            "connectivity": connectivity, "raw_filepath": mesh_path, "raw_description_filepath": info_path, "raw_instance_filepath": agg_path,
            "raw_segmentation_filepath": seg_path, "raw_label_filepath": label_path if has_gt else None}


def mesh_only_points_table(xyz, rgb, normals, segment_ids):
    """arkit_preprocessing.py:102-116 -> f32[N,12]: xyz, rgb 0..255, normal, segment id, label 0, instance -1, stacked
    in f64 and rounded once."""
    n = np.asarray(xyz).shape[0]
    labels = np.stack([np.zeros(n, np.int64), np.full(n, -1, np.int64)], 1)
    return np.hstack([np.asarray(xyz, np.float64), np.asarray(rgb, np.float64), np.asarray(normals, np.float64),
                      np.asarray(segment_ids, np.int64)[:, None], labels]).astype(np.float32)


def _load_pseudo_files(scene, pseudo_dir):
    """-> (cloud, masks) of a scene, or None with the reference's message when a file is missing."""
    try:
        return (np.load(os.path.join(pseudo_dir, f"{scene}_cloud.npy")),
                np.load(os.path.join(pseudo_dir, f"{scene}_masks.npy")))
    except FileNotFoundError as e:
        print(f"Could not load pseudo masks for {scene}: {e.filename}")
        return None


def _frameless_tables(m, scene, raw_path, cloud, masks, dev, normals=None):
    """The tables of a scan without frames or ground truth from its loaded dict `m` (`scans.load_mesh_only_scan` /
    `load_point_cloud_scan`): the cloud file must equal m["xyz"] bit for bit in f32, the masks are taken row for row.
    normals: f32[N,3] to store, None to estimate them from the points."""
    xyz = m["xyz"].astype(np.float32)
    if cloud.ndim != 2 or cloud.shape[1] < 3 or cloud.shape[0] != xyz.shape[0] or \
            not np.array_equal(np.ascontiguousarray(cloud[:, :3], dtype=np.float32).view(np.uint32), xyz.view(np.uint32)):
        raise ValueError(f"{scene}: {scene}_cloud.npy {list(cloud.shape)} is not the scan's {xyz.shape[0]} kept vertices "
                         f"row for row (was it written from a scene file of this scan with the same --segments-min-verts?)")
    if masks.ndim != 2 or masks.shape[0] != xyz.shape[0]:
        raise ValueError(f"{scene}: pseudo masks {list(masks.shape)} do not match the cloud's {xyz.shape[0]} points")
    if normals is None:
        normals = ops.estimate_normals(torch.from_numpy(xyz).to(dev), 0.1, 30).cpu().numpy()
    mean, second = color_moments(m["rgb"])
    return {"points": mesh_only_points_table(xyz, m["rgb"], normals, m["segment_ids"]),
            "freemasks": masks.astype(np.float32), "gt": None, "color_mean": mean, "color_std": second, "connectivity": m["seg_connectivity"], "raw_filepath": raw_path,
            "raw_description_filepath": "", "raw_instance_filepath": "", "raw_segmentation_filepath": "",
            "raw_label_filepath": None, "scene": scene}


def build_point_cloud_tables(scan, pseudo_dir, device="cuda", segments_min_verts=scans.POINTS_SEGMENTS_MIN_VERTS,
                             segment_dimension_order=0, graph_k=8, graph_radius=0.1, small_segments="merge"):
    """One point-cloud scan -> the dict of `build_mesh_only_tables`, or None (with a message) when its pseudo-mask files
    are missing.  xyz, colours and segment ids are `scans.load_point_cloud_scan`'s (same graph arguments as the scene
    file was written with); the normals are the file's when it has them, else `ops.estimate_normals(xyz, 0.1, 30)`."""
    dev = torch.device(device)
    scene, cloud_path = scans.point_cloud_scan_path(scan)
    files = _load_pseudo_files(scene, pseudo_dir)
    if files is None:
        return None
    m = scans.load_point_cloud_scan(scan, segments_min_verts, segment_dimension_order, graph_k, graph_radius,
                                    small_segments, device=dev)
    return _frameless_tables(m, scene, cloud_path, *files, dev, m["normals"] if m["normals_from_file"] else None)


def build_mesh_only_tables(scan, pseudo_dir, device="cuda", segments_min_verts=scans.ARKIT_SEGMENTS_MIN_VERTS,
                           segment_dimension_order=0):
    """One mesh-only scan -> the dict of `build_scene_tables` (gt None, connectivity of the written level), or None
    (with a message) when its pseudo-mask files are missing — arkit_preprocessing.py `process_file`, with the module
    docstring's deviation: xyz, colours and segment ids are `scans.load_mesh_only_scan`'s, the cloud file must equal xyz
    bit for bit, the masks are taken row for row, the normals are `ops.estimate_normals(xyz, 0.1, 30)`."""
    dev = torch.device(device)
    scene, mesh_path = scans.mesh_only_scan_path(scan)
    files = _load_pseudo_files(scene, pseudo_dir)
    if files is None:
        return None
    m = scans.load_mesh_only_scan(scan, segments_min_verts, segment_dimension_order, device=dev)
    return _frameless_tables(m, scene, mesh_path, *files, dev)


def color_moments(rgb):
    """A scene's database entries `color_mean` / `color_std` (:162-171) from its colours 0..255 (f64 [N,3]): per channel
    the mean of c / 255 and the mean of (c / 255)^2 — the second moment, under the reference's name."""
    c = np.asarray(rgb, np.float64)
    return ([float((c[:, j] / 255).mean()) for j in range(3)], [float(((c[:, j] / 255) ** 2).mean()) for j in range(3)])


def color_mean_std(database):
    """`compute_color_mean_std` (:222-240) of a list of database entries -> {"mean": [3], "std": [3]}: the mean of the
    scenes' means, sqrt(mean of the scenes' second moments - mean^2), scenes weighted equally."""
    mean = np.array([e["color_mean"] for e in database]).mean(axis=0)
    std = np.sqrt(np.array([e["color_std"] for e in database]).mean(axis=0) - mean ** 2)
    return {"mean": [float(v) for v in mean], "std": [float(v) for v in std]}


def save_yaml(path, obj):
    import yaml

    with open(path, "w") as f:
        yaml.safe_dump(obj, f, default_style=None, default_flow_style=False)


def build_dataset(scans_root, split_files, pseudo_dir, out_dir, oracle=False, device="cuda",
                  foreground_ids=FOREGROUND_CLASS_IDS, segments_min_verts=None, write_connectivity=False,
                  layout="scannet", segment_dimension_order=0, graph_k=8, graph_radius=0.1, small_segments="merge"):
    """`split_files`: {mode: text file with one scan name per line} (ScanNet's scannetv2_train.txt / _val.txt), or
    {mode: list of names}.  Every scan `scans_root/<name>` of a mode goes through `build_scene_tables`; scans without
    pseudo-mask files are skipped with a message.  Writes the files the module docstring lists.
    `write_connectivity`: a scan whose segment ids come from the over-segmentation also gets
    `{mode}/0000_00_connectivity.npy` (int32[P,2]) and the entry keys `connectivity_filepath` and
    `segments_min_verts`, which spare `FreeMaskSceneReader(resegment_mesh=True)` its per-item segmentation; a scan
    with a segs.json has no adjacency to store and says so.
    `segments_min_verts`: None is 20 (layout="scannet") or scans.ARKIT_SEGMENTS_MIN_VERTS (layout="arkit").
    layout="arkit": mesh-only scans through `build_mesh_only_tables` (module docstring); names are ARKitScenes' scene
    ids (a sub-directory or a .ply file of `scans_root`), files are `{mode}/{scene}.npy`, entries carry
    `scene_type: room` and empty raw description / instance / segmentation paths; `oracle` is refused.
    layout="points": point-cloud scans through `build_point_cloud_tables` with `graph_k`, `graph_radius` and
    `small_segments` (`segments_min_verts` None is scans.POINTS_SEGMENTS_MIN_VERTS); everything else as for "arkit".
    -> {mode: list of database entries}."""
    if layout not in scans.LAYOUTS:
        raise ValueError(f"build_dataset: layout must be 'scannet', 'arkit' or 'points', got {layout!r}")
    arkit = layout != "scannet"                       # frame-less scans without ground truth: "arkit" and "points"
    if arkit and oracle:
        raise ValueError(f"build_dataset(layout={layout!r}): such scans have no ground truth for oracle masks")
    if segments_min_verts is None:
        segments_min_verts = {"scannet": 20, "arkit": scans.ARKIT_SEGMENTS_MIN_VERTS,
                              "points": scans.POINTS_SEGMENTS_MIN_VERTS}[layout]
    out_dir = os.fspath(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    save_yaml(os.path.join(out_dir, "label_database.yaml"), LABEL_DATABASE)
    databases = {}
    for mode, split in split_files.items():
        if isinstance(split, (str, os.PathLike)):
            with open(split) as f:
                split = [line.strip() for line in f if line.strip()]
        names = sorted(split)
        for name in names:
            if not arkit:
                parse_scene_dir(name)                 # a bad name fails before anything is written for the mode
        os.makedirs(os.path.join(out_dir, mode), exist_ok=True)
        database = []
        for name in names:
            scan_dir = os.path.join(os.fspath(scans_root), name)
            if layout == "points":
                t = build_point_cloud_tables(scan_dir, pseudo_dir, device=device, segments_min_verts=segments_min_verts,
                                             segment_dimension_order=segment_dimension_order, graph_k=graph_k,
                                             graph_radius=graph_radius, small_segments=small_segments)
            elif arkit:
                t = build_mesh_only_tables(scan_dir, pseudo_dir, device=device, segments_min_verts=segments_min_verts,
                                           segment_dimension_order=segment_dimension_order)
            else:
                t = build_scene_tables(scan_dir, pseudo_dir, oracle=oracle, device=device, foreground_ids=foreground_ids,
                                       segments_min_verts=segments_min_verts)
            if t is None:
                continue
            if arkit:
                scene, sub = t["scene"], 0            # arkit_preprocessing.py:168-169
                path = os.path.join(out_dir, mode, f"{scene}.npy")
            else:
                _, scene, sub = parse_scene_dir(scan_dir)
                path = os.path.join(out_dir, mode, f"{scene:04}_{sub:02}.npy")
            np.save(path, t["points"])
            mask_path = path.replace(".npy", "_freemasks.npy")
            np.save(mask_path, t["freemasks"])
            entry = {"filepath": path, "scene": scene, "sub_scene": sub, "raw_filepath": t["raw_filepath"],
                     "file_len": int(t["points"].shape[0]), "color_mean": t["color_mean"], "color_std": t["color_std"],
                     "freemask_filepath": mask_path}
            if arkit:
                entry["scene_type"] = "room"          # the reference's placeholders for what ARKit has not (:107-111)
            for key in ("raw_description_filepath", "raw_instance_filepath", "raw_segmentation_filepath",
                        "raw_label_filepath"):
                if t[key] is not None:
                    entry[key] = t[key]
            if write_connectivity and t["connectivity"] is not None:
                conn_path = path.replace(".npy", "_connectivity.npy")
                np.save(conn_path, np.asarray(t["connectivity"], np.int32).reshape(-1, 2))
                entry["connectivity_filepath"] = conn_path
                entry["segments_min_verts"] = int(np.atleast_1d(segments_min_verts)[segment_dimension_order if arkit else 0])
            elif write_connectivity:
                print(f"{name}: segment ids come from {t['raw_segmentation_filepath']}, no connectivity to write")
            if t["gt"] is not None:
                gt_path = os.path.join(out_dir, "instance_gt", mode, f"scene{scene:04}_{sub:02}.txt")
                os.makedirs(os.path.dirname(gt_path), exist_ok=True)
                np.savetxt(gt_path, t["gt"], fmt="%d")
                entry["instance_gt_filepath"] = gt_path
            database.append(entry)
        save_yaml(os.path.join(out_dir, f"{mode}_database.yaml"), database)
        databases[mode] = database
    stats_from = databases.get("train") or databases.get("validation") or next(iter(databases.values()), [])
    if stats_from:
        save_yaml(os.path.join(out_dir, "color_mean_std.yaml"), color_mean_std(stats_from))
    return databases
