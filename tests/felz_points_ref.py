"""Reference, scenes and file writers of the point-cloud over-segmentation tests (tests/test_felz_points_host.py,
tests/test_gpu_felz_points.py): DESIGN.md §3.30 restated in numpy and plain Python.

    knn_edges_ref       the edge rule, with Python sets
    edge_weights_ref    both weight modes in float32, every operation rounded on its own (numpy float32 arithmetic has
                        no fused multiply-add), the colour threshold compared in float64
    merge_ref           the two merge loops over sorted edges, a plain union-find
    segment_points_ref  k-NN (normals_ref.knn_hybrid_f64) -> edges -> weights -> stable sort -> merge
    merge_floaters_ref  the small_segments="merge" rule with a brute-force nearest point

Partitions are compared after `first_occurrence` renumbering: representatives differ between union-find variants."""
import numpy as np

from knn_ref import knn1_f64
from normals_ref import knn_hybrid_f64

F = np.float32


# ------------------------------------------------------------------------------------------------------------- edges
def knn_edges_ref(idx, count):
    """-> (edge_a i32[E], edge_b i32[E]) in (row, position) order."""
    idx, count = np.asarray(idx), np.asarray(count)
    listed = [set(int(j) for j in idx[i, :count[i]]) for i in range(idx.shape[0])]
    a, b = [], []
    for i in range(idx.shape[0]):
        for p in range(int(count[i])):
            j = int(idx[i, p])
            if j == i:
                continue
            if i < j or i not in listed[j]:            # the lower row speaks for a mutual pair
                a.append(i)
                b.append(j)
    return np.array(a, np.int32), np.array(b, np.int32)


# ----------------------------------------------------------------------------------------------------------- weights
def _dot3(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def edge_weights_ref(points, colors, normals, edge_a, edge_b, oriented):
    """f32[E].  oriented: (1 - n_a.n_b) * L1 colour distance, squared when the far normal has a positive component along
    the edge and the colour distance is below 0.05 (as a double).  Not oriented: (1 - |n_a.n_b|) * colour distance."""
    P, C, N = (np.asarray(x, F) for x in (points, colors, normals))
    a, b = np.asarray(edge_a, np.int64), np.asarray(edge_b, np.int64)
    dot = _dot3(N[a], N[b])
    normal_dist = F(1) - (dot if oriented else np.abs(dot))
    diff = np.abs(C[a] - C[b])
    color_dist = (diff[:, 0] + diff[:, 1]) + diff[:, 2]
    w = normal_dist * color_dist
    if oriented:
        with np.errstate(invalid="ignore", divide="ignore"):
            d = P[b] - P[a]
            length = np.sqrt(_dot3(d, d))
            d = d / length[:, None]                    # a zero-length edge: NaN, and NaN > 0 is False
            along = _dot3(N[b], d)
            square = (along > 0) & (color_dist.astype(np.float64) < 0.05)
        w = np.where(square, w * w, w)
    assert w.dtype == F
    return w


# ------------------------------------------------------------------------------------------------------------- merge
def merge_ref(edge_a, edge_b, weights, n, kthr, min_verts):
    """Edges in non-decreasing weight order -> root of every vertex, i64[n]."""
    root = list(range(n))
    size = [1] * n
    limit = [F(kthr)] * n

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    def union(x, y):
        if size[x] < size[y]:
            x, y = y, x
        root[y] = x
        size[x] += size[y]
        return x

    for a, b, w in zip(edge_a.tolist(), edge_b.tolist(), np.asarray(weights, F)):
        ra, rb = find(a), find(b)
        if ra != rb and w <= limit[ra] and w <= limit[rb]:
            r = union(ra, rb)
            limit[r] = F(w + F(kthr) / F(size[r]))
    for a, b in zip(edge_a.tolist(), edge_b.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb and (size[ra] < min_verts or size[rb] < min_verts):
            union(ra, rb)
    return np.array([find(v) for v in range(n)], np.int64)


def first_occurrence(labels):
    """Renumber labels 0, 1, .. in the order in which they first appear -> i64[n]."""
    labels = np.asarray(labels)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse.reshape(-1)].astype(np.int64)


def symmetric_connectivity(labels, edge_a, edge_b):
    """Sorted set of (s(a), s(b)) and (s(b), s(a)) over the edges that join two segments, i64[P,2]."""
    pairs = set()
    for a, b in zip(np.asarray(edge_a).tolist(), np.asarray(edge_b).tolist()):
        if labels[a] != labels[b]:
            pairs.add((int(labels[a]), int(labels[b])))
            pairs.add((int(labels[b]), int(labels[a])))
    return np.array(sorted(pairs), np.int64).reshape(-1, 2)


def renumbered(labels, connectivity):
    """(labels, connectivity) of any implementation in first-occurrence numbering, pairs sorted."""
    labels = np.asarray(labels)
    new = first_occurrence(labels)
    table = np.full(int(labels.max()) + 1, -1, np.int64)
    table[labels] = new
    conn = table[np.asarray(connectivity, np.int64).reshape(-1, 2)]
    return new, np.array(sorted(map(tuple, conn.tolist())), np.int64).reshape(-1, 2)


def graph_ref(points, colors, normals, oriented, k, radius):
    """-> (edge_a, edge_b, weights) sorted by weight, equal weights in (row, position) order."""
    idx, count = knn_hybrid_f64(points, points, k + 1, radius)
    a, b = knn_edges_ref(idx, count)
    w = edge_weights_ref(points, colors, normals, a, b, oriented)
    order = np.argsort(w, kind="stable")
    return a[order], b[order], w[order]


def segment_points_ref(points, colors, normals, oriented, k, radius, kthr=0.005, min_verts=20):
    """-> (labels i64[N] in first-occurrence numbering, connectivity i64[P,2], (edge_a, edge_b, weights) sorted)."""
    a, b, w = graph_ref(points, colors, normals, oriented, k, radius)
    labels = first_occurrence(merge_ref(a, b, w, len(points), kthr, min_verts))
    return labels, symmetric_connectivity(labels, a, b), (a, b, w)


def merge_floaters_ref(labels, connectivity, min_verts, points):
    """A segment smaller than min_verts, or absent from the connectivity, takes the segment of the point nearest to its
    first row among the points of the other (kept) segments; none kept -> all 0.  -> i64[N], not renumbered."""
    labels = np.asarray(labels, np.int64)
    named = set(np.asarray(connectivity).reshape(-1).tolist())
    ids = sorted(set(labels.tolist()))
    floaters = [s for s in ids if (labels == s).sum() < min_verts or s not in named]
    if len(floaters) == len(ids):
        return np.zeros_like(labels)
    kept_rows = np.nonzero(~np.isin(labels, floaters))[0]
    out = labels.copy()
    for s in floaters:
        first = int(np.nonzero(labels == s)[0][0])
        j, _ = knn1_f64(points[first:first + 1], points[kept_rows])
        out[labels == s] = labels[kept_rows[int(j[0])]]
    return out


# ------------------------------------------------------------------------------------------------------------ scenes
TWO_PLANES = dict(k=8, radius=0.12, kthr=0.005, min_verts=20)
FLOOR_RGB, WALL_RGB = (0.8, 0.2, 0.2), (0.2, 0.2, 0.8)


def two_planes(seed=0, cluster=False):
    """Two 20 x 20 grids at 0.05 spacing with in-plane jitter +-0.01: a floor at z = 0 (normal +z) and a wall at x = 0
    that starts 0.05 above the floor (normal +x), rows permuted.  cluster: 5 more points 1 m from the planes, in the rows
    behind the permuted planes.  -> (points f32[N,3], colors f32[N,3], normals f32[N,3], plane i64[N]: 0 floor, 1 wall,
    2 cluster)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2) * 0.05
    floor = np.concatenate([g + rng.uniform(-0.01, 0.01, g.shape), np.zeros((400, 1))], 1)
    wall = np.concatenate([np.zeros((400, 1)), g + [0.0, 0.05] + rng.uniform(-0.01, 0.01, g.shape)], 1)
    points = np.concatenate([floor, wall])
    colors = np.concatenate([np.tile(FLOOR_RGB, (400, 1)), np.tile(WALL_RGB, (400, 1))])
    normals = np.concatenate([np.tile((0.0, 0.0, 1.0), (400, 1)), np.tile((1.0, 0.0, 0.0), (400, 1))])
    plane = np.repeat([0, 1], 400)
    perm = rng.permutation(800)
    points, colors, normals, plane = points[perm], colors[perm], normals[perm], plane[perm]
    if cluster:
        blob = np.array([0.5, 2.0, 0.3]) + rng.uniform(-0.02, 0.02, (5, 3))      # 1 m behind the floor's far edge
        points = np.concatenate([points, blob])
        colors = np.concatenate([colors, np.tile((0.1, 0.9, 0.1), (5, 1))])
        normals = np.concatenate([normals, np.tile((0.0, 1.0, 0.0), (5, 1))])
        plane = np.concatenate([plane, np.full(5, 2)])
    return points.astype(F), colors.astype(F), normals.astype(F), plane.astype(np.int64)


def random_cloud(n, seed):
    """n points uniform in the unit cube, 24 of them copies of earlier rows (coincident points); colours from a palette
    of four plus noise of 0.01, so that many neighbours differ by less than 0.05; random unit normals."""
    rng = np.random.default_rng(seed)
    points = rng.random((n, 3))
    dup = rng.choice(n, 24, replace=False)
    points[dup] = points[(dup * 7 + 3) % n]
    palette = np.array([[0.2, 0.3, 0.4], [0.21, 0.3, 0.41], [0.7, 0.1, 0.1], [0.5, 0.5, 0.5]])
    colors = palette[rng.integers(0, 4, n)] + rng.uniform(-0.01, 0.01, (n, 3))
    normals = rng.normal(size=(n, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    return points.astype(F), colors.astype(F), normals.astype(F)


RANDOM_RADIUS = 0.08      # 2048 points per unit volume: 4.4 neighbours expected, so rows of every length 1 .. 9


def coincident_four():
    """Rows 0, 1, 3 at one place, row 2 0.05 away: in row 3 the point itself comes third (ties go by index)."""
    points = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.55, 0.5, 0.5], [0.5, 0.5, 0.5]], F)
    colors = np.array([[0.1, 0.2, 0.3], [0.12, 0.2, 0.3], [0.9, 0.2, 0.3], [0.1, 0.21, 0.3]], F)
    normals = np.array([[0, 0, 1], [0, 0.6, 0.8], [1, 0, 0], [0, 0, -1]], F)
    return points, colors, normals


# ------------------------------------------------------------------------------------------------------------- files
def write_ply_points(path, points, rgb, normals=None, faces=None, fmt="binary_little_endian"):
    """A PLY file with a vertex element (x y z [nx ny nz] red green blue, colours uchar) and, with `faces`, a face
    element behind it."""
    points, rgb = np.asarray(points, F), np.asarray(rgb, np.uint8)
    n = points.shape[0]
    head = ["ply", f"format {fmt} 1.0", f"element vertex {n}", "property float x", "property float y", "property float z"]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        head += ["property float nx", "property float ny", "property float nz"]
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    head += ["property uchar red", "property uchar green", "property uchar blue"]
    fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if faces is not None:
        head += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
    head.append("end_header")
    rec = np.zeros(n, np.dtype(fields))
    for j, name in enumerate("xyz"):
        rec[name] = points[:, j]
    if normals is not None:
        for j, name in enumerate(("nx", "ny", "nz")):
            rec[name] = np.asarray(normals, F)[:, j]
    for j, name in enumerate(("red", "green", "blue")):
        rec[name] = rgb[:, j]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if fmt == "ascii":
            for row in rec:
                f.write((" ".join(repr(float(v)) if isinstance(v, np.floating) else str(int(v)) for v in row) + "\n").encode())
            for face in ([] if faces is None else faces):
                f.write(("3 " + " ".join(str(int(v)) for v in face) + "\n").encode())
        else:
            f.write(rec.tobytes())
            if faces is not None:
                frec = np.zeros(len(faces), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
                frec["n"], frec["v"] = 3, np.asarray(faces, np.int32)
                f.write(frec.tobytes())
