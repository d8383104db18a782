"""Shared inputs and numpy restatements for the dataset tests (test_dataset_host.py, test_gpu_dataset.py): PLY / scan
directory writers, the mask-table cases, float64 vertex normals and `process_file` restated."""
import json
import os

import numpy as np

FOREGROUND = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)


# ----------------------------------------------------------------------------------------------------------- writers
def write_ply(path, xyz, rgb=None, faces=None, label=None, fmt="binary_little_endian", rgb_type="uchar"):
    """A ScanNet-style PLY: x y z (float), optional red green blue (+ alpha 255 when uchar), optional `label` (ushort),
    faces with a uchar count."""
    V = xyz.shape[0]
    faces = np.zeros((0, 3), np.int32) if faces is None else faces
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = ["ply", f"format {fmt} 1.0", "comment written by tests/dataset_cases.py", f"element vertex {V}",
            "property float x", "property float y", "property float z"]
    if rgb is not None:
        for n in ("red", "green", "blue"):
            head.append(f"property {rgb_type} {n}")
            fields.append((n, "u1" if rgb_type == "uchar" else "<f4"))
        if rgb_type == "uchar":
            head.append("property uchar alpha")
            fields.append(("alpha", "u1"))
    if label is not None:
        head.append("property ushort label")
        fields.append(("label", "<u2"))
    head += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rec = np.zeros(V, dtype=np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgb is not None:
        rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
        if rgb_type == "uchar":
            rec["alpha"] = 255
    if label is not None:
        rec["label"] = label
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if fmt == "ascii":
            for r in rec:
                f.write((" ".join(repr(float(v)) if np.asarray(v).dtype.kind == "f" else str(int(v)) for v in r) + "\n").encode())
            for t in faces:
                f.write(f"3 {t[0]} {t[1]} {t[2]}\n".encode())
        else:
            f.write(rec.tobytes())
            frec = np.zeros(faces.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
            frec["n"], frec["i"] = 3, faces
            f.write(frec.tobytes())


AXIS = np.array([[0.8, -0.6, 0.0, 1.25], [0.6, 0.8, 0.0, -0.5], [0.0, 0.0, 1.0, 0.125], [0.0, 0.0, 0.0, 1.0]])


def write_scan(root, name, seed, side=14, gt=True, segs=True, fmt="binary_little_endian", axis=AXIS):
    """A scan directory from `synthetic.make_mesh(seed, side)`: mesh with uchar colours, info file with axisAlignment,
    and (gt) labels PLY, segs.json with NON-contiguous segment numbers, aggregation.json.  -> dict of what was written."""
    from unscene3d_amd.synthetic import make_mesh

    rng = np.random.default_rng(seed)
    vertices, faces, colors = make_mesh(seed, side=side)[:3]
    V = vertices.shape[0]
    rgb = np.clip(np.rint(colors * 255), 0, 255).astype(np.uint8)
    d = os.path.join(root, name)
    os.makedirs(d, exist_ok=True)
    write_ply(os.path.join(d, f"{name}_vh_clean_2.ply"), vertices, rgb, faces, fmt=fmt)
    with open(os.path.join(d, f"{name}.txt"), "w") as f:
        if axis is not None:
            f.write("axisAlignment = " + " ".join(repr(float(v)) for v in axis.reshape(-1)) + "\n")
        f.write("colorHeight = 968\nsceneType = Office\n")
    out = {"dir": d, "vertices": vertices, "faces": faces, "rgb": rgb, "axis": np.identity(4) if axis is None else axis}
    u, v = np.divmod(np.arange(V), side)
    seg_raw = ((u // 4) * 10 + (v // 4)) * 7 + 3                 # blocks of 4 x 4 vertices, sparse numbering
    if segs:
        with open(os.path.join(d, f"{name}_vh_clean_2.0.010000.segs.json"), "w") as f:
            json.dump({"sceneId": name, "segIndices": seg_raw.tolist()}, f)
        out["segIndices"] = seg_raw
    if gt:
        uniq = np.unique(seg_raw)
        parts = np.array_split(rng.permutation(uniq), 5)
        # classes of the five groups: chair 5, table 7, wall 1 (outside the list), cabinet 3, otherfurniture 39; the last
        # segments stay without a group
        classes = [5, 7, 1, 3, 39]
        groups = [{"id": i, "objectId": i, "segments": parts[i][:-1].tolist() if i == 4 else parts[i].tolist(),
                   "label": str(classes[i])} for i in range(5)]
        label = np.full(V, 2, np.int64)                           # floor where no group reaches
        label[np.isin(seg_raw, parts[4][-1:])] = 40              # an id outside the list on an ungrouped segment
        for g, c in zip(groups, classes):
            label[np.isin(seg_raw, g["segments"])] = c
        with open(os.path.join(d, f"{name}.aggregation.json"), "w") as f:
            json.dump({"sceneId": name, "segGroups": groups}, f)
        write_ply(os.path.join(d, f"{name}_vh_clean_2.labels.ply"), vertices, rgb, faces, label=label, fmt=fmt)
        out.update(label=label, groups=groups)
    return out


def write_pseudo(pseudo_dir, name, scan, seed, K=6, soft=False, compact=False):
    """`{name}_cloud.npy` / `_masks.npy`: the cloud is a shuffled copy of the aligned vertices, jittered by < 1 mm
    (grid spacing 50 mm: the nearest neighbour is never in doubt).  Masks: random entries (bool, or f32 with `soft`),
    or with `compact` K discs of a quarter of the scene's width around random cloud points (masks that pass the
    reader's extent filter)."""
    rng = np.random.default_rng(seed + 77)
    v = scan["vertices"].astype(np.float64)
    aligned = np.hstack([v, np.ones((v.shape[0], 1))]) @ scan["axis"].T[:, :3]
    perm = rng.permutation(v.shape[0])
    cloud = (aligned[perm] + rng.uniform(-1e-3, 1e-3, aligned.shape)).astype(np.float32)
    masks = rng.uniform(0, 1, (v.shape[0], K)).astype(np.float32) if soft else rng.uniform(0, 1, (v.shape[0], K)) < 0.3
    if compact:
        radius = 0.25 * float(np.ptp(cloud[:, 0]))
        centres = cloud[rng.choice(cloud.shape[0], K, replace=False), :2]
        masks = np.linalg.norm(cloud[:, None, :2] - centres[None], axis=-1) < radius
    os.makedirs(pseudo_dir, exist_ok=True)
    np.save(os.path.join(pseudo_dir, f"{name}_cloud.npy"), cloud)
    np.save(os.path.join(pseudo_dir, f"{name}_masks.npy"), masks)
    return cloud, masks


# ------------------------------------------------------------------------------------------------------ restatements
def vertex_normals_f64(vertices, faces):
    """open3d's compute_vertex_normals restated in float64 numpy, faces added in ascending order (corner order within
    a face): -> (normals f64[V,3], bound f64[V]).  bound = 8 (deg + 8) 2^-53 T / |sum| per component, T = the sum of
    the magnitudes of every product that entered the vertex's sum (all three components: the normalisation couples
    them), deg = number of corners added; 0 where the answer is the exact (0,0,1)."""
    P = vertices.astype(np.float64)
    V = P.shape[0]
    s = np.zeros((V, 3))
    T = np.zeros(V)
    deg = np.zeros(V, np.int64)
    for f in faces:
        a, b = P[f[1]] - P[f[0]], P[f[2]] - P[f[0]]
        n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        t = (abs(a[1] * b[2]) + abs(a[2] * b[1]) + abs(a[2] * b[0]) + abs(a[0] * b[2]) + abs(a[0] * b[1])
             + abs(a[1] * b[0]))
        for v in f:
            s[v] += n
            T[v] += t
            deg[v] += 1
    norm = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
    ok = norm > 0
    out = np.tile(np.array([0.0, 0.0, 1.0]), (V, 1))
    out[ok] = s[ok] / norm[ok, None]
    bound = np.zeros(V)
    bound[ok] = 8.0 * (deg[ok] + 8) * 2.0 ** -53 * T[ok] / norm[ok]
    return out, bound


def scene_tables_numpy(scan, cloud=None, masks=None, oracle=False):
    """`process_file` (freemask_preprocessing.py:66-220) in numpy from what `write_scan` returned, brute-force 1-NN.
    -> (points f64[N,12] with the float64 normals, normal bound, freemasks f32, gt int32 or None, color_mean, color_std)."""
    coords = scan["vertices"]
    normals, bound = vertex_normals_f64(coords, scan["faces"])
    features = np.hstack([scan["rgb"].astype(np.float64), normals])
    points = np.hstack([coords, features])
    segments = scan["segIndices"]
    points = np.hstack([points, np.unique(segments, return_inverse=True)[1].reshape(-1, 1)])
    if "label" in scan:
        labels = np.hstack([scan["label"].astype(np.uint32)[:, None], np.full((len(coords), 1), -1)])
        for inst in scan["groups"]:
            labels[np.isin(segments, np.array(inst["segments"])), 1] = inst["id"]
        fg = np.isin(labels[:, 0], FOREGROUND)
        labels[fg, 0] = 1
        labels[~fg, 1] = -1
    else:
        labels = np.hstack([np.zeros((len(coords), 1), np.int64), np.full((len(coords), 1), -1)])
    points = np.hstack([points, labels])
    gt = (points[:, -2] * 1000 + points[:, -1] + 1).astype(np.int32) if "label" in scan else None
    mean = [float((features[:, j] / 255).mean()) for j in range(3)]
    std = [float(((features[:, j] / 255) ** 2).mean()) for j in range(3)]
    if oracle:
        n = len(set(np.unique(labels[:, 1])) - {-1})
        free = np.zeros((len(coords), n), np.float32)
        for i in range(n):
            free[labels[:, 1] == i, i] = 1.0
    else:
        homo = np.hstack([points[:, :3], np.ones((len(coords), 1))])
        aligned = homo @ scan["axis"].T[:, :3]
        d2 = ((aligned[:, None, :] - cloud[None, :, :3].astype(np.float64)) ** 2).sum(-1)
        free = masks[d2.argmin(1)].astype(np.float32)
    return points, bound, free, gt, mean, std


# -------------------------------------------------------------------------------------------------- mask-table cases
TABLE_SHAPES = ((1, 1), (70, 3), (257, 33), (300, 65), (5000, 50))
FEATURES = ("empty", "wide_x", "wide_y", "limit", "at_thr", "last_row")


def mask_table_cases(N, K, thr, ratio=0.8, seed=0):
    """-> list of (coordinates f32[N,3], soft f32[N,K], segments f32[N], {feature: column}) for one shape.  The six
    special columns (FEATURES) are dealt to the K columns; a shape with K < 6 gets ceil(6 / K) variants so that every
    feature occurs at that shape.  Scene extent: x in [0, 10], y in [0, 20] (rows 0 and 1 pin the corners); with
    s = f32(extent) * f32(ratio), rows 2 .. 5 sit at x = s, x = next(s), y = s_y, y = next(s_y).  With N < 8 the rows
    that do not exist are left out and a feature means what is left of it (N = 1: one point, every extent is 0)."""
    rng = np.random.default_rng(seed + 31 * N + K)
    t = np.float32(thr)
    below, above = np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2))
    xyz = np.stack([rng.uniform(0.5, 7.5, N), rng.uniform(0.5, 15.5, N), rng.uniform(0, 3, N)], 1).astype(np.float32)
    sx = np.float32(10) * np.float32(ratio)
    sy = np.float32(20) * np.float32(ratio)
    special = [(0, 0), (10, 20), (sx, 1), (np.nextafter(sx, np.float32(99)), 1), (1, sy), (1, np.nextafter(sy, np.float32(99)))]
    for r, (x, y) in enumerate(special[:N]):
        xyz[r, 0], xyz[r, 1] = x, y
    if N > len(special):
        xyz[N - 1, :2] = (3, 3)
    segments = rng.integers(0, 40, N).astype(np.float32)
    cases = []
    for variant in range(-(-len(FEATURES) // K)):
        # ordinary columns: ~20 % of the rows of the inner box set, soft values anywhere in [0, 1]
        soft = rng.uniform(0, 1, (N, K)).astype(np.float32)
        soft[rng.uniform(0, 1, (N, K)) < 0.6] *= np.float32(0.3)
        soft[:min(N, len(special))] = below                       # ordinary columns leave the pinned rows alone
        where = {}
        for j in range(K):
            i = variant * K + j
            if i >= len(FEATURES):
                break
            feat = FEATURES[i]
            col = (j * 7) % K if K >= len(FEATURES) else j        # spread over the tiles of a wide table
            while col in where.values():
                col = (col + 1) % K
            where[feat] = col
            soft[:, col] = rng.uniform(0, float(below), N).astype(np.float32)
            rows = {"empty": [], "wide_x": [0, 3], "wide_y": [0, 5], "limit": [0, 2, 4], "at_thr": [],
                    "last_row": [N - 1]}[feat]
            for r in rows:
                if r < N:
                    soft[r, col] = above if r % 2 else np.float32(0.9)
            if feat == "empty":
                soft[::3, col] = t                                # exactly at the threshold: not set
                soft[1::3, col] = below
            if feat == "at_thr":
                soft[:, col] = t
                soft[N // 2:, col] = below
                if N > len(special) + 1:
                    soft[len(special):len(special) + 1, col] = above      # one row just above: the only hit
        cases.append((xyz, soft, segments, where))
    return cases


def host_tables(xyz, soft, segments, thr, ratio, device):
    """The default reader's lines (`filter_by_extent` + datasets/freemask.py `__getitem__`) -> (table i32 or None, keep)."""
    from unscene3d_amd.datasets.freemask import filter_by_extent

    keep = filter_by_extent(xyz, soft, thr, ratio, device)
    if not keep:
        return None, keep
    hard = soft[:, keep] > thr
    table = np.concatenate([hard.any(1).astype(np.int32).reshape(-1, 1), hard.astype(np.int32)], axis=1)
    return np.hstack((table, segments[..., None].astype(table.dtype))).astype(np.int32), keep
