"""ScanNet-style scan directories -> the scene files tools/pseudo_masks_run.py reads (reference
pseudo_masks/datasets/scannet.py: `load_intrinsics` :199-216, `load_rgb_data` :126-154, `segment_mesh` :156-197,
`prepare_scene_data` :234-283, voxelised by pseudo_masks/datasets/voxelizer.py:109-148).

A scan directory `DIR/{scene}/` holds what the reference reads under `scannet_images_path/{scene}/`:

    {scene}.txt               `key = value` lines: axisAlignment, colorHeight / colorWidth, fx/fy/mx/my_color
    {scene}_vh_clean_2.ply    the coloured triangle mesh
    color/*.jpg | *.png | *.npy   colour frames (.npy: uint8 [H, W, 3], already at the target size)
    pose/*.txt                one 4x4 camera-to-world matrix per frame

The readers are numpy only; Pillow is imported when a frame is a .jpg / .png, and only then.  The reference reads the
same files through open3d, plyfile and torchvision.  `build_scene` joins the readers with the stages of the package:
voxelisation (ME.utils.sparse_quantize), the mesh over-segmentation (felzenszwalb_cpp.segment_mesh), the image encoder
and the ray-cast projection (pipeline.encode_scene_feats_2d).

The 3D modality: with `model_3d` (a Res16UNet34CMultiRes, e.g. models.weights.load_csc_backbone on the published CSC
checkpoint) `build_scene` runs the voxels through the backbone and carries the features of level `res_{resolution_scale}`
to every voxel (`pipeline.encode_scene_feats_3d`; reference unscene3d_pseudo_main.py:332-348) as `feats_3d`.  With
`images=False`, or for a scan directory that has neither `color/` nor `pose/`, no frame is read and the file holds the
geometry modality alone (the reference's `modality: geom`).

Mesh-only scans (`layout="arkit"`; reference pseudo_masks/datasets/arkit.py:61-144): a scan is
`DIR/{scene}/{scene}_3dod_mesh.ply` (ARKitScenes' naming) or a flat `DIR/{scene}.ply`, with no info file, no axis
alignment and no frames.  `load_mesh_only_scan` cleans the mesh, over-segments it at several sizes, drops the vertices
of too-small segments and shifts the rest to the origin; `build_scene` then runs the same voxelisation and 3D backbone
and writes a geometry-only scene file.

Point-cloud scans (`layout="points"`): a scan is `DIR/{scene}/{scene}.ply` or a flat `DIR/{scene}.ply`
with a vertex element only (S3DIS rooms, laser scans, LiDAR).  `load_point_cloud_scan` over-segments the cloud on its
k-NN graph (`felzenszwalb_cpp.segment_points`; the reference reconstructs a Poisson mesh first,
pseudo_masks/datasets/preprocess/stanford.py:80-135), and `build_scene` writes a geometry-only scene file as for a
mesh-only scan.

Not covered: depth
images, label / instance columns (the training dataset's builder, datasets/preprocessing.py, reads them through
`read_ply_vertex_properties`), chunked scenes, S3DIS's annotation folders and images for point-cloud scans."""
from __future__ import annotations

import glob
import os

import numpy as np

PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
             "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
             "double": "f8", "float64": "f8"}
FRAME_SUFFIXES = (".jpg", ".png", ".npy")
ARKIT_SEGMENTS_MIN_VERTS = (50, 100, 150, 200)     # segments_min_vert_nums of the reference's ARKit configuration
ARKIT_MESH_SUFFIX = "_3dod_mesh.ply"
POINTS_SEGMENTS_MIN_VERTS = (50,)                  # layout="points": one level unless the caller asks for more
SMALL_SEGMENTS = ("merge", "drop", "keep")         # load_point_cloud_scan(small_segments=...)
LAYOUTS = ("scannet", "arkit", "points")
SCENE_NN_3D = "grid"     # the 1-NN of build_scene's 3D branch: what profiles/knn1_grid.txt measured faster


# ---------------------------------------------------------------------------------------------------- info and poses
def read_scan_info(path, align=True):
    """`{scene}.txt` (scannet.py:199-216): one `key = value` per line, numeric values as float arrays.
    -> dict with axisAlignment f64[4,4] (identity when the key is absent or `align` is False, :210), colorHeight,
    colorWidth (int), fx_color, fy_color, mx_color, my_color (float), and every other key as the reference keeps it (a
    float array; text values, which the reference turns into empty arrays, stay strings)."""
    info = {}
    with open(path) as f:
        for line in f:
            if " = " not in line:
                continue
            key, val = line.split(" = ", 1)
            try:
                info[key.strip()] = np.array([float(t) for t in val.split()], np.float64)
            except ValueError:
                info[key.strip()] = val.strip()
    axis = info.get("axisAlignment")
    if align and isinstance(axis, np.ndarray):
        if axis.size != 16:
            raise ValueError(f"{path}: axisAlignment has {axis.size} values, expected 16")
        info["axisAlignment"] = axis.reshape(4, 4)
    else:
        info["axisAlignment"] = np.identity(4)
    for key, cast in (("colorHeight", int), ("colorWidth", int), ("fx_color", float), ("fy_color", float),
                      ("mx_color", float), ("my_color", float)):
        v = info.get(key)
        if not isinstance(v, np.ndarray) or v.size != 1:
            raise ValueError(f"{path}: needs one number for {key}")
        info[key] = cast(v[0])
    return info


def read_pose(path):
    """A 4x4 matrix as text, one row per line (utils/utils.py `load_matrix_from_txt`) -> f64[4,4].  ScanNet writes
    `-inf` in every entry of a frame whose tracking was lost; those parse to non-finite values."""
    with open(path) as f:
        vals = [float(t) for t in f.read().split()]
    if len(vals) != 16:
        raise ValueError(f"{path}: {len(vals)} values, expected a 4x4 matrix")
    return np.array(vals, np.float64).reshape(4, 4)


def color_intrinsics(info, shape_hw):
    """fx, fy, mx, my of the colour camera at the target image size, f64[4], as scannet.py:133-138 scales them:
    color_scale = (H / colorHeight, W / colorWidth) and fx, mx take color_scale[0], fy, my take color_scale[1].  That
    pairs fx and mx with the HEIGHT ratio and fy and my with the WIDTH ratio — the other way round from the axes they
    belong to.  It is kept because the reference's features were produced with it; ScanNet's 1296x968 frames resized to
    256x192 have ratios 0.1983 and 0.1975, so the two pairings differ by 0.4 %."""
    H, W = shape_hw
    scale = (H / info["colorHeight"], W / info["colorWidth"])
    return np.array([info["fx_color"] * scale[0], info["fy_color"] * scale[1], info["mx_color"] * scale[0],
                     info["my_color"] * scale[1]], np.float64)


# --------------------------------------------------------------------------------------------------------------- PLY
def _ply_header(f, path):
    if f.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError(f"{path}: PLY header has no end_header")
        t = line.decode("ascii", "replace").split()
        if not t or t[0] in ("comment", "obj_info"):
            continue
        if t[0] == "end_header":
            break
        if t[0] == "format":
            fmt = t[1]
        elif t[0] == "element":
            elements.append((t[1], int(t[2]), []))
        elif t[0] == "property":
            if not elements:
                raise ValueError(f"{path}: PLY property before the first element")
            types = t[2:4] if t[1] == "list" else t[1:2]
            if any(ty not in PLY_TYPES for ty in types):
                raise ValueError(f"{path}: unknown PLY property type in {' '.join(t)!r}")
            elements[-1][2].append(("list", t[2], t[3], t[4]) if t[1] == "list" else ("scalar", t[1], t[2]))
        else:
            raise ValueError(f"{path}: unknown PLY header line {' '.join(t)!r}")
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not covered (binary_little_endian and ascii are)")
    return fmt, elements


def _face_layout(props, path):
    """The face element's record with every list holding 3 entries: (numpy dtype, name of the index field)."""
    lists = [p for p in props if p[0] == "list"]
    if len(lists) != 1 or lists[0][3] not in ("vertex_indices", "vertex_index"):
        raise ValueError(f"{path}: the face element needs exactly one list property, vertex_indices")
    if lists[0][1] not in ("uchar", "uint8", "int", "int32"):
        raise ValueError(f"{path}: face list count type {lists[0][1]!r} is not covered (uchar and int are)")
    fields = []
    for p in props:
        if p[0] == "list":
            fields += [("_count", "<" + PLY_TYPES[p[1]]), ("_index", "<" + PLY_TYPES[p[2]], (3,))]
        else:
            fields.append((p[2], "<" + PLY_TYPES[p[1]]))
    return np.dtype(fields)


def read_ply_mesh(path):
    """A coloured triangle mesh -> (vertices f32[V,3], colors f32[V,3] in [0,1], faces i32[F,3]); what the reference
    takes from open3d's read_triangle_mesh (scannet.py:163-176).

    Formats `binary_little_endian` and `ascii`.  Vertex properties are scalars of any standard PLY type (x, y, z, red,
    green, blue are used, the others skipped; integer colours are divided by 255).  The face element has one list
    property `vertex_indices` with a `uchar` or `int` count, and scalars beside it are skipped; the file is read as
    fixed-size records of three indices, so a mesh of triangles never takes a per-face loop.  A face that is not a
    triangle, another format (big endian) or an unknown property type raises ValueError with the file name."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        vertex = faces = None
        for name, count, props in elements:
            if name == "face":
                dt = _face_layout(props, path)
            else:
                if any(p[0] == "list" for p in props):
                    raise ValueError(f"{path}: list property in element {name!r} is not covered")
                dt = np.dtype([(p[2], "<" + PLY_TYPES[p[1]]) for p in props])
            if fmt == "binary_little_endian":
                buf = f.read(dt.itemsize * count)
                rec = np.frombuffer(buf[:len(buf) // dt.itemsize * dt.itemsize], dtype=dt)
                if name != "face" and rec.shape[0] != count:      # a short face element may be a face with > 3 indices
                    raise ValueError(f"{path}: element {name!r} ends after {rec.shape[0]} of {count} records")
            else:
                rows = [f.readline().decode("ascii", "replace").split() for _ in range(count)]
                width = sum(int(np.prod(dt[n].shape, dtype=np.int64)) for n in dt.names)
                if name == "face":
                    bad = [i for i, r in enumerate(rows) if not r or int(r[0]) != 3]
                    if bad:
                        raise ValueError(f"{path}: face {bad[0]} is not a triangle "
                                         f"({rows[bad[0]][0] if rows[bad[0]] else 'no'} vertices)")
                if any(len(r) != width for r in rows):
                    raise ValueError(f"{path}: element {name!r} has a line that does not hold {width} values")
                table = np.array(rows, dtype=np.float64).reshape(count, width)
                rec = np.zeros(count, dtype=dt)
                col = 0
                for n in dt.names:
                    w = int(np.prod(dt[n].shape, dtype=np.int64))
                    rec[n] = table[:, col:col + w].reshape((count,) + dt[n].shape)
                    col += w
            if name == "vertex":
                vertex = rec
            elif name == "face":
                counts = rec["_count"]
                bad = np.nonzero(counts != 3)[0]
                if bad.size:
                    raise ValueError(f"{path}: face {int(bad[0])} is not a triangle ({int(counts[bad[0]])} vertices)")
                if rec.shape[0] != count:
                    raise ValueError(f"{path}: element 'face' ends after {rec.shape[0]} of {count} records")
                faces = rec["_index"]
    if vertex is None or faces is None:
        raise ValueError(f"{path}: needs a vertex and a face element")
    for n in ("x", "y", "z", "red", "green", "blue"):
        if n not in vertex.dtype.names:
            raise ValueError(f"{path}: vertex property {n!r} is missing")
    vertices = np.stack([vertex["x"], vertex["y"], vertex["z"]], 1).astype(np.float32)
    rgb = [vertex[n] for n in ("red", "green", "blue")]
    colors = np.stack([c.astype(np.float64) / 255.0 if c.dtype.kind in "iu" else c.astype(np.float64) for c in rgb], 1)
    if faces.size and (faces.min() < 0 or faces.max() >= vertices.shape[0]):
        raise ValueError(f"{path}: face index outside [0, {vertices.shape[0]})")
    return vertices, colors.astype(np.float32), np.ascontiguousarray(faces, dtype=np.int32)


def read_ply_vertex_properties(path, names):
    """Scalar properties of the vertex element as they are stored -> {name: array[V]} in the property's own type (what
    the reference takes from plyfile's `elements[0].data[name]`): the integer colours 0..255 of a mesh, the `label` of
    ScanNet's `*_vh_clean_2.labels.ply`.  Same formats as `read_ply_mesh`.  Elements in front of the vertex element
    must hold scalars only (they are skipped).  A missing property or vertex element raises ValueError with the file
    name."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        for name, count, props in elements:
            if any(p[0] == "list" for p in props):
                raise ValueError(f"{path}: list property in element {name!r} (the vertex element or one in front of "
                                 f"it) is not covered")
            dt = np.dtype([(p[2], "<" + PLY_TYPES[p[1]]) for p in props])
            if fmt == "binary_little_endian":
                buf = f.read(dt.itemsize * count)
                if len(buf) != dt.itemsize * count:
                    raise ValueError(f"{path}: element {name!r} ends after {len(buf) // max(1, dt.itemsize)} of {count} records")
                rec = np.frombuffer(buf, dtype=dt)
            else:
                rows = [f.readline().decode("ascii", "replace").split() for _ in range(count)]
                if any(len(r) != len(dt.names) for r in rows):
                    raise ValueError(f"{path}: element {name!r} has a line that does not hold {len(dt.names)} values")
                table = np.array(rows, dtype=np.float64).reshape(count, len(dt.names))
                rec = np.zeros(count, dtype=dt)
                for col, n in enumerate(dt.names):
                    rec[n] = table[:, col]
            if name == "vertex":
                missing = [n for n in names if n not in dt.names]
                if missing:
                    raise ValueError(f"{path}: vertex property {missing[0]!r} is missing")
                return {n: np.ascontiguousarray(rec[n]) for n in names}
    raise ValueError(f"{path}: needs a vertex element")


def read_ply_points(path):
    """A coloured point cloud -> (points f32[N,3], colors f32[N,3] in [0,1], normals f32[N,3] or None).

    Only the vertex element is needed, with x, y, z, red, green, blue (integer colours are divided by 255, as in
    `read_ply_mesh`); nx, ny, nz are read when all three are there, else normals is None.  A face element, or any other
    element behind the vertex element, is ignored — a mesh file is a valid point cloud.  Same formats and header rules
    as `read_ply_vertex_properties`, which reads the records."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        _, elements = _ply_header(f, path)
    have = [p[2] for name, _, props in elements if name == "vertex" for p in props if p[0] == "scalar"]
    names = ["x", "y", "z", "red", "green", "blue"]
    with_normals = all(n in have for n in ("nx", "ny", "nz"))
    v = read_ply_vertex_properties(path, names + (["nx", "ny", "nz"] if with_normals else []))
    points = np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)
    rgb = [v[n] for n in ("red", "green", "blue")]
    colors = np.stack([c.astype(np.float64) / 255.0 if c.dtype.kind in "iu" else c.astype(np.float64) for c in rgb], 1)
    normals = np.stack([v["nx"], v["ny"], v["nz"]], 1).astype(np.float32) if with_normals else None
    return points, colors.astype(np.float32), normals


# ------------------------------------------------------------------------------------------------------------ frames
def frame_files(color_dir, pose_dir, every=1):
    """-> [(colour file, pose file)] in the reference's order: `sorted()` of the file names of each directory, paired by
    position (scannet.py:142,149).  `sorted()` is LEXICOGRAPHIC: frames 0, 20, 100 come as 0, 100, 20.  The order is
    kept because the scene features are a running pairwise mean over the frames (a later frame weighs more), so another
    order gives other features.  The two lists must hold the same frame names; `every` keeps every k-th pair."""
    colors = sorted((p for s in FRAME_SUFFIXES for p in glob.glob(os.path.join(color_dir, "*" + s))),
                    key=os.path.basename)
    poses = sorted(glob.glob(os.path.join(pose_dir, "*.txt")), key=os.path.basename)
    stem = lambda p: os.path.splitext(os.path.basename(p))[0]
    if [stem(p) for p in colors] != [stem(p) for p in poses]:
        raise ValueError(f"{color_dir} and {pose_dir} do not hold the same frames "
                         f"({len(colors)} colour files, {len(poses)} poses)")
    return list(zip(colors, poses))[::max(1, int(every))]


def load_image(path, shape_hw):
    """One colour frame -> f32[3,H,W] in [-1, 1]: resized to (H, W) as scannet.py:122 does
    (`Image.open(p).convert('RGB').resize((W, H), Image.BILINEAR)`), then / 255 (:144) and (x - 0.5) / 0.5 (:115).  A
    .npy frame is uint8 [H, W, 3] at the target size already and needs no Pillow."""
    H, W = shape_hw
    if path.endswith(".npy"):
        rgb = np.load(path)
        if rgb.dtype != np.uint8 or rgb.shape != (H, W, 3):
            raise ValueError(f"{path}: a .npy frame must be uint8 [{H}, {W}, 3], got {rgb.dtype} {list(rgb.shape)}")
    else:
        from PIL import Image
        rgb = np.array(Image.open(path).convert("RGB").resize((W, H), Image.BILINEAR))
    x = (rgb / 255.0).astype(np.float32)
    x = (x - np.float32(0.5)) / np.float32(0.5)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def load_frames(color_dir, pose_dir, shape_hw, every=1, axis_alignment=None):
    """-> (images f32[n,3,H,W], poses f64[n,4,4], n_dropped): the frames of `frame_files` (lexicographic order, see
    there) as `load_image` reads them, with poses `axis_alignment @ pose` (scannet.py:152).  The intrinsics that go with
    `shape_hw` come from `color_intrinsics`, which keeps the reference's pairing of fx with the height ratio.

    Deviation: a frame whose pose is not finite (ScanNet writes -inf where tracking was lost) is dropped and counted in
    n_dropped.  The reference casts such frames too; every ray of one is NaN and hits nothing."""
    H, W = shape_hw
    axis = np.identity(4) if axis_alignment is None else np.asarray(axis_alignment, np.float64)
    images, poses, dropped = [], [], 0
    for color_file, pose_file in frame_files(color_dir, pose_dir, every):
        pose = read_pose(pose_file)
        if not np.isfinite(pose).all():
            dropped += 1
            continue
        images.append(load_image(color_file, shape_hw))
        poses.append(axis @ pose)
    if not images:
        return np.zeros((0, 3, H, W), np.float32), np.zeros((0, 4, 4), np.float64), dropped
    return np.stack(images), np.stack(poses), dropped


# ---------------------------------------------------------------------------------------------------- mesh-only scans
def clean_mesh(vertices, colors, faces):
    """arkit.py:61-87: drop the vertices no face references and re-index the faces.
    -> (vertices[kept], colors[kept], faces i32[F,3] into the kept rows, kept i64[V'] ascending)."""
    vertices, colors, faces = np.asarray(vertices), np.asarray(colors), np.asarray(faces, np.int32).reshape(-1, 3)
    kept = np.unique(faces)
    removed = np.ones(vertices.shape[0], np.int64)
    removed[kept] = 0
    shift = np.cumsum(removed)                         # unreferenced vertices in front of, or at, each vertex
    return vertices[kept], colors[kept], (faces - shift[faces]).astype(np.int32), kept.astype(np.int64)


def clean_segments(comps, min_vert_num=500):
    """arkit.py:89-93: -> (comps[valid], valid bool[V]) with valid = the vertex's segment has at least `min_vert_num`
    vertices."""
    comps = np.asarray(comps)
    ids, counts = np.unique(comps, return_counts=True)
    valid = ~np.isin(comps, ids[counts < min_vert_num])
    return comps[valid], valid


def mesh_only_scan_path(scan, suffix=ARKIT_MESH_SUFFIX):
    """-> (scene name, mesh file) of a mesh-only scan: the directory `DIR/{scene}` holding `{scene}_3dod_mesh.ply`, or
    the flat file `DIR/{scene}.ply`.  `suffix`: what the file inside a directory is called after the scene name."""
    scan = os.path.normpath(os.fspath(scan))
    if os.path.isdir(scan):
        scene = os.path.basename(scan)
        return scene, os.path.join(scan, scene + suffix)
    if scan.endswith(".ply"):
        return os.path.basename(scan)[:-4], scan
    return os.path.basename(scan), scan + ".ply"


def mesh_only_scans(root):
    """The scans of a directory in the mesh-only layout, sorted by scene name: sub-directories and *.ply files."""
    found = {}
    for e in os.listdir(root):
        p = os.path.join(root, e)
        if os.path.isdir(p) or e.endswith(".ply"):
            found[mesh_only_scan_path(p)[0]] = p
    return [found[k] for k in sorted(found)]


def load_mesh_only_scan(scan, segments_min_verts=ARKIT_SEGMENTS_MIN_VERTS, segment_dimension_order=0, device="cuda"):
    """`ARKit_Dataset.load_mesh` + `load_scene_data` (arkit.py:95-144), the deterministic mesh stages of a mesh-only
    scan -> dict:

        scene             str
        mesh_path         str
        xyz               f64[N,3]   kept vertices minus their minimum (:142)
        rgb               f64[N,3]   colours * 255 (:104); integer colours of the file are exact
        segments          i64[N,L]   the over-segmentation at every level, kept rows
        segment_ids       i64[N]     column `segment_dimension_order`
        seg_connectivity  i64[E,2]   that level's directed segment pairs
        kept              i64[N]     rows of the file's vertex element

    The mesh is cleaned (`clean_mesh`), then `felzenszwalb_cpp.segment_mesh(vertices, faces, colours * 255, 0.005, n)`
    runs for every n of `segments_min_verts` on the whole cleaned mesh (the edge weights are computed and sorted once;
    each level is one host merge).  As the reference is written, `clean_segments` runs at every level but only the
    vertex mask of the LAST level decides which vertices stay: a vertex stays when its segment at the last level has at
    least segments_min_verts[-1] vertices.  Deviation: connectivity pairs that name a segment left without vertices are
    dropped (the reference keeps them; nothing refers to such a segment)."""
    import torch

    from .. import felzenszwalb_cpp as felz

    levels = tuple(int(n) for n in np.atleast_1d(segments_min_verts))
    if not levels or not 0 <= int(segment_dimension_order) < len(levels):
        raise ValueError(f"segment_dimension_order {segment_dimension_order} is no level of segments_min_verts {levels}")
    scene, mesh_path = mesh_only_scan_path(scan)
    vertices, colors, faces = read_ply_mesh(mesh_path)
    vertices, colors, faces, kept = clean_mesh(vertices, colors, faces)
    if vertices.shape[0] == 0:
        raise ValueError(f"{mesh_path}: no vertex is referenced by a face")
    rgb = colors.astype(np.float64) * 255.0
    whole = np.rint(rgb)                               # integer colours come back as 199.99999: undo the trip through
    rgb = np.where(np.abs(rgb - whole) < 1e-3, whole, rgb)          # f32 [0, 1], which the dataset's uint8 cast would cut
    dev = torch.device(device)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt).contiguous()
    ea, eb, w, _ = felz.edge_weights(to(vertices, torch.float32), to(faces, torch.int32), to(rgb, torch.float32))
    order = torch.sort(w, stable=True).indices                      # as felzenszwalb_cpp.segment_mesh orders them
    sa, sb, sw = ea[order].cpu().numpy(), eb[order].cpu().numpy(), w[order].cpu().numpy()
    segments, connectivity, valid = [], [], None
    for n in levels:
        seg, conn = felz.relabel(felz.merge_host(sa, sb, sw, vertices.shape[0], 0.005, n), sa, sb)
        segments.append(seg)
        connectivity.append(conn)
        _, valid = clean_segments(seg, min_vert_num=n)              # the last level's mask is the one that is used
    segments = np.stack(segments, -1).astype(np.int64)[valid]
    xyz = vertices[valid].astype(np.float64)
    xyz -= xyz.min(0)
    level = int(segment_dimension_order)
    conn = np.asarray(connectivity[level], np.int64).reshape(-1, 2)
    conn = conn[np.isin(conn, np.unique(segments[:, level])).all(1)]
    return {"scene": scene, "mesh_path": mesh_path, "xyz": xyz, "rgb": rgb[valid], "segments": segments,
            "segment_ids": np.ascontiguousarray(segments[:, level]), "seg_connectivity": conn, "kept": kept[valid]}


# -------------------------------------------------------------------------------------------------- point-cloud scans
def point_cloud_scan_path(scan):
    """-> (scene name, cloud file) of a point-cloud scan: `DIR/{scene}/{scene}.ply` or the flat file `DIR/{scene}.ply`."""
    return mesh_only_scan_path(scan, ".ply")


def point_cloud_scans(root):
    """The scans of a directory in the point-cloud layout, sorted by scene name: sub-directories and *.ply files."""
    return mesh_only_scans(root)


def _check_point_cloud_args(segments_min_verts, segment_dimension_order, graph_k, graph_radius, small_segments):
    levels = tuple(int(n) for n in np.atleast_1d(segments_min_verts))
    if not levels or not 0 <= int(segment_dimension_order) < len(levels):
        raise ValueError(f"segment_dimension_order {segment_dimension_order} is no level of segments_min_verts {levels}")
    if small_segments not in SMALL_SEGMENTS:
        raise ValueError(f"small_segments must be one of {SMALL_SEGMENTS}, got {small_segments!r}")
    if not 0 <= int(graph_k) <= 63:
        raise ValueError(f"graph_k must be 0 .. 63, got {graph_k}")
    if not (float(graph_radius) > 0 and np.isfinite(float(graph_radius))):
        raise ValueError(f"graph_radius must be a positive finite number, got {graph_radius!r}")
    return levels


def merge_floaters(labels, connectivity, min_verts, nearest):
    """stanford.py:114-128 with the deviation below: a segment with fewer than `min_verts` points, or one that no
    connectivity pair names, is a floater the graph never reached; it takes the segment of the nearest point of a KEPT
    (non-floater) segment, measured from the floater's first row.  labels i[N]; connectivity i[P,2];
    nearest(query_rows i64[Q], ref_rows i64[R]) -> i64[Q], positions in ref_rows.  -> labels i64[N], not renumbered.
    Deviation: the reference takes the nearest point of ANY other segment, which can be another floater, so the result
    depends on the order of the loop; here a floater always lands in a kept segment.  No kept segment: all 0."""
    labels = np.asarray(labels, np.int64)
    ids, first, counts = np.unique(labels, return_index=True, return_counts=True)
    floater = (counts < int(min_verts)) | ~np.isin(ids, np.asarray(connectivity, np.int64).reshape(-1))
    if not floater.any():
        return labels.copy()
    if floater.all():
        return np.zeros_like(labels)
    ref_rows = np.nonzero(np.isin(labels, ids[~floater]))[0]
    target = labels[ref_rows[np.asarray(nearest(first[floater], ref_rows), np.int64)]]
    table = np.arange(int(ids.max()) + 1, dtype=np.int64)
    table[ids[floater]] = target
    return table[labels]


def load_point_cloud_scan(scan, segments_min_verts=POINTS_SEGMENTS_MIN_VERTS, segment_dimension_order=0, graph_k=8,
                          graph_radius=0.1, small_segments="merge", device="cuda"):
    """A coloured point cloud without a mesh (S3DIS rooms, laser scans, LiDAR) -> the dict of `load_mesh_only_scan`:

        scene, cloud_path  str
        xyz               f64[N,3]   kept points minus their minimum
        rgb               f64[N,3]   colours * 255
        segments          i64[N,L]   `felzenszwalb_cpp.segment_points` at every level of `segments_min_verts`, kept rows
        segment_ids       i64[N]     column `segment_dimension_order`
        seg_connectivity  i64[E,2]   that level's segment pairs, both directions
        kept              i64[N]     rows of the file's vertex element
        normals           f32[N,3]   kept rows: the file's nx, ny, nz, or `ops.estimate_normals` of the file's points
        normals_from_file bool

    The scan is `DIR/{scene}/{scene}.ply` or a flat `DIR/{scene}.ply` (`read_ply_points`).  The graph is
    `felzenszwalb_cpp.point_graph(points, colours in [0, 1], normals of the file or None, graph_k, graph_radius)` — the
    colour scale stanford.py:107-112 passes — built and sorted ONCE; every level is one host merge with kthr 0.005.
    graph_k=8 and graph_radius=0.1 are unmeasured starting values.
    small_segments, per level with its minimum n:
        "merge"  `merge_floaters` (stanford.py:114-128 and its documented deviation), the nearest point through
                 `ops.knn1_grid`; labels are renumbered and the connectivity recomputed from the edge list.  All rows stay.
        "drop"   arkit's rule (`clean_segments`, `load_mesh_only_scan`): the rows of segments below the LAST level's
                 minimum are removed, `kept` says which stay, pairs naming a removed segment are dropped.
        "keep"   nothing; all rows stay.
    The reference reconstructs a Poisson mesh and segments that (stanford.py:80-135); see DESIGN.md §3.30."""
    import torch

    from .. import felzenszwalb_cpp as felz
    from .. import ops

    levels = _check_point_cloud_args(segments_min_verts, segment_dimension_order, graph_k, graph_radius, small_segments)
    scene, cloud_path = point_cloud_scan_path(scan)
    points, colors, file_normals = read_ply_points(cloud_path)
    n_points = points.shape[0]
    if n_points == 0:
        raise ValueError(f"{cloud_path}: the vertex element is empty")
    rgb = colors.astype(np.float64) * 255.0
    whole = np.rint(rgb)                               # as load_mesh_only_scan: integer colours come back exact
    rgb = np.where(np.abs(rgb - whole) < 1e-3, whole, rgb)
    dev = torch.device(device)
    points_d = torch.from_numpy(points).to(dev)
    normals_d = ops.estimate_normals(points_d) if file_normals is None else torch.from_numpy(file_normals).to(dev)
    sa, sb, sw = felz.point_graph(points_d, colors, normals_d, graph_k, graph_radius, device=dev,
                                  oriented=file_normals is not None)

    def nearest(query_rows, ref_rows):
        q = points_d[torch.from_numpy(query_rows).to(dev)].contiguous()
        r = points_d[torch.from_numpy(ref_rows).to(dev)].contiguous()
        return ops.knn1_grid(q, r)[1].cpu().numpy()

    segments, connectivity, valid = [], [], np.ones(n_points, bool)
    for n in levels:
        seg, conn = felz.relabel_symmetric(felz.merge_host(sa, sb, sw, n_points, 0.005, n), sa, sb)
        if small_segments == "merge":
            seg, conn = felz.relabel_symmetric(merge_floaters(seg, conn, n, nearest), sa, sb)
        elif small_segments == "drop":
            _, valid = clean_segments(seg, min_vert_num=n)          # the last level's mask is the one that is used
        segments.append(seg)
        connectivity.append(conn)
    if not valid.any():
        raise ValueError(f"{cloud_path}: no segment has {levels[-1]} points; nothing is left with small_segments='drop'")
    segments = np.stack(segments, -1).astype(np.int64)[valid]
    xyz = points[valid].astype(np.float64)
    xyz -= xyz.min(0)
    level = int(segment_dimension_order)
    conn = np.asarray(connectivity[level], np.int64).reshape(-1, 2)
    conn = conn[np.isin(conn, np.unique(segments[:, level])).all(1)]
    return {"scene": scene, "cloud_path": cloud_path, "xyz": xyz, "rgb": rgb[valid], "segments": segments,
            "segment_ids": np.ascontiguousarray(segments[:, level]), "seg_connectivity": conn,
            "kept": np.nonzero(valid)[0].astype(np.int64), "normals": normals_d.cpu().numpy()[valid],
            "normals_from_file": file_normals is not None}


# ------------------------------------------------------------------------------------------------------------- scene
def build_scene(scan_dir, model, voxel_size=0.02, image_hw=(192, 256), segments_min_verts=None, frame_batch=None,
                attention=False, every=1, align=True, device="cuda", model_3d=None, resolution_scale=2,
                precision_3d="f32", images=True, layout="scannet", segment_dimension_order=0, graph_k=8,
                graph_radius=0.1, small_segments="merge"):
    """One scan directory -> the arrays of a scene file (tools/pseudo_masks_run.py), as the reference's dataset and
    `encode_scene_feats` produce them at test time (no augmentation):

        coords            i32[N,4]   (0, x, y, z) voxel coordinates
        colors            f32[N,3]   rgb / 255 - 0.5 of the kept vertices (scannet.py:281): the 3D backbone's input
        feats_2d          f32[N,C]   running mean of the image features over the frames; all-zero rows = not seen
        feats_2d_query    f32[N,C]   only with `attention`
        feats_3d          f32[N,C3]  only with `model_3d`: its `res_{resolution_scale}` features (96 channels at res_2)
        resolution_scale  int        only with `model_3d`
        segment_ids       i64[N]     felzenszwalb_cpp.segment_mesh(vertices, faces, colors, 0.005, segments_min_verts or 50)
        seg_connectivity  i64[E,2]
        full_res_coords   f32[M,3]   the aligned mesh vertices, metres
        voxel_size        float
        frames_used, frames_dropped  int

    The points are the mesh vertices, aligned with axisAlignment (:213-214).  They are voxelised as voxelizer.py:132-148
    does with augmentation off and no clip bound: floor(xyz * (1 / voxel_size)) in float64 — a product with the
    reciprocal, as the voxelisation matrix has it, not a division — and ME.utils.sparse_quantize(return_index=True).
    Deviations: the kept row of a voxel is its FIRST vertex and the rows keep vertex order (this package's
    sparse_quantize; the reference's MinkowskiEngine leaves the order to its hash map); the reference takes a vertex's
    segment through a 1-NN search of the points against the mesh vertices (:186-191), which is the identity here since
    the points are those vertices; frames with a non-finite pose are dropped (`load_frames`).
    The camera translations are divided by the voxel size (:255-258; no rotation at test time), the frames run through
    `pipeline.encode_scene_feats_2d(model, ..., frame_batch=frame_batch)` with `model` a models.encoders_2d.DinoNet.

    model_3d: a Res16UNet34CMultiRes in eval mode.  The voxels go through it as SparseTensor(colors, coords) — the
    arrays above — with the convolutions in `precision_3d` ("f32" or "bf16"), and `pipeline.encode_scene_feats_3d`
    carries the level's features to the voxels by exact 1-NN through the grid kernel (ops.knn1_grid).
    images=False, or a scan directory with neither `color/` nor `pose/`: no frame is read, `model` may be None, and
    `feats_2d`, `frames_used` and `frames_dropped` are not written — a geometry-only scene file.  That needs `model_3d`;
    `images=False` without it raises before anything is read.  A directory that has the frame folders but no usable
    frame still gets `feats_2d` as zeros.

    layout="arkit": `scan_dir` is a mesh-only scan (`load_mesh_only_scan`; `segments_min_verts` is then the tuple of
    levels, None meaning ARKIT_SEGMENTS_MIN_VERTS, and `segment_dimension_order` picks the level that is written).  There is no
    info file, no alignment and no frame: it needs `model_3d`, the file is geometry-only (no `feats_2d`), the points
    are the kept vertices shifted to the origin, `colors` is rgb / 255 - 0.5 of the kept voxels as above and
    `full_res_coords` is the kept, shifted vertices in f32.  layout="scannet", the default, is everything above.

    layout="points": `scan_dir` is a point-cloud scan (`load_point_cloud_scan` with `graph_k`, `graph_radius`,
    `small_segments`; `segments_min_verts` None means POINTS_SEGMENTS_MIN_VERTS).  Frame-less like "arkit" in every
    respect above: it needs `model_3d`, the file is geometry-only, the points are the kept points shifted to the
    origin.  Images for point-cloud scans are not covered."""
    import torch

    if layout not in LAYOUTS:
        raise ValueError(f"build_scene: layout must be 'scannet', 'arkit' or 'points', got {layout!r}")
    if layout != "scannet":
        images = False
    if not images and model_3d is None:
        raise ValueError("build_scene(images=False) needs model_3d: the scene file would hold no features")

    from .. import MinkowskiEngine as ME
    from .. import felzenszwalb_cpp
    from ..project_features_cuda import Project2DFeaturesCUDA
    from .pipeline import encode_scene_feats_2d, encode_scene_feats_3d

    dev = torch.device(device)
    if layout == "arkit":
        levels = ARKIT_SEGMENTS_MIN_VERTS if segments_min_verts is None else segments_min_verts
        m = load_mesh_only_scan(scan_dir, levels, segment_dimension_order, device=dev)
        xyz, colors = m["xyz"], (m["rgb"] / 255.0).astype(np.float32)
        seg, conn, info, axis = m["segment_ids"], m["seg_connectivity"], None, None
    elif layout == "points":
        levels = POINTS_SEGMENTS_MIN_VERTS if segments_min_verts is None else segments_min_verts
        m = load_point_cloud_scan(scan_dir, levels, segment_dimension_order, graph_k, graph_radius, small_segments,
                                  device=dev)
        xyz, colors = m["xyz"], (m["rgb"] / 255.0).astype(np.float32)
        seg, conn, info, axis = m["segment_ids"], m["seg_connectivity"], None, None
    else:
        scene = os.path.basename(os.path.normpath(scan_dir))
        info = read_scan_info(os.path.join(scan_dir, f"{scene}.txt"), align=align)
        axis = info["axisAlignment"]
        vertices, colors, faces = read_ply_mesh(os.path.join(scan_dir, f"{scene}_vh_clean_2.ply"))   # scannet.py:163
        homo = np.hstack([vertices.astype(np.float64), np.ones((vertices.shape[0], 1))])
        xyz = homo @ axis.T[:, :3]

    grid = np.floor(xyz * (1.0 / voxel_size)).astype(np.int32)
    _, kept = ME.utils.sparse_quantize(grid, return_index=True, device=dev)
    kept = kept.cpu().numpy()
    coords = np.concatenate([np.zeros((kept.shape[0], 1), np.int32), grid[kept]], 1)

    if layout == "scannet":
        seg, conn = felzenszwalb_cpp.segment_mesh(xyz.astype(np.float32), faces, colors, 0.005,
                                                  50 if segments_min_verts is None else int(segments_min_verts), device=dev)

    H, W = image_hw
    color_dir, pose_dir = os.path.join(scan_dir, "color"), os.path.join(scan_dir, "pose")
    if model_3d is not None and not os.path.isdir(color_dir) and not os.path.isdir(pose_dir):
        images = False                                              # a scan without frames: geometry only
    if images and model is None:
        raise ValueError(f"{scan_dir}: has frames, so build_scene needs the image encoder `model` (or images=False)")
    out = {"coords": coords, "colors": (colors[kept] - np.float32(0.5)).astype(np.float32)}
    coords_d = torch.from_numpy(coords).to(dev)
    counts = {}
    if images:
        frames, poses, dropped = load_frames(color_dir, pose_dir, image_hw, every=every, axis_alignment=axis)
        poses = poses.copy()
        poses[:, :3, 3] /= voxel_size
        feats = None
        if frames.shape[0]:
            projecter = Project2DFeaturesCUDA(width=W, height=H, voxel_size=voxel_size)
            intr = torch.from_numpy(color_intrinsics(info, image_hw).astype(np.float32)).to(dev).view(1, 4)
            feats = encode_scene_feats_2d(model, torch.from_numpy(frames).to(dev).unsqueeze(0),
                                          torch.from_numpy(poses.astype(np.float32)).to(dev).unsqueeze(0), intr,
                                          coords_d, projecter, attention=attention, frame_batch=frame_batch)
        if feats is None:                                           # no usable frame: nothing was seen
            zeros = torch.zeros((coords.shape[0], int(model.feature_dim)), dtype=torch.float32)
            feats = (zeros, zeros.clone()) if attention else zeros
        key, query = feats if attention else (feats, None)
        out["feats_2d"] = key.cpu().numpy()
        if attention:
            out["feats_2d_query"] = query.cpu().numpy()
        counts = dict(frames_used=int(frames.shape[0]), frames_dropped=int(dropped))
    if model_3d is not None:
        sinput = ME.SparseTensor(features=torch.from_numpy(out["colors"]).to(dev), coordinates=coords_d, device=dev)
        out["feats_3d"] = encode_scene_feats_3d(model_3d, sinput, resolution_scale=int(resolution_scale),
                                                precision=precision_3d, nn=SCENE_NN_3D).float().cpu().numpy()
        out["resolution_scale"] = int(resolution_scale)
    out.update(segment_ids=seg[kept].astype(np.int64), seg_connectivity=np.asarray(conn, np.int64).reshape(-1, 2),
               full_res_coords=xyz.astype(np.float32), voxel_size=float(voxel_size), **counts)
    return out
