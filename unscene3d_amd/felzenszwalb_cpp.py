"""`felzenszwalb_cpp.segment_mesh` of the reference (pybind11 module built from utils/cpp_utils/segmentator.cpp:156-250;
called by pseudo_masks/datasets/scannet.py:176): graph-based over-segmentation of a coloured triangle mesh into
geometrically consistent segments + the directed segment adjacency.

    seg_indices, seg_connectivity = felzenszwalb_cpp.segment_mesh(vertices f32[V,3], faces i32[F,3], colors f32[V,3],
                                                                  kthr=0.005, segMinVerts=20)
    -> (i32[V] labels 0..S-1, i32[P,2] pairs (segment of a, segment of b) over the mesh edges, lexicographically sorted)

Normals, edge weights and the edge sort run on the MI355X (csrc/felz.hip, bit-equal weights); the two sequential
merge loops run on the host inside the library (usc_felz_merge_host).  Equal weights keep face order (stable sort)
where the reference's std::sort leaves their order to libstdc++: the partition is the same, the label NUMBERS (ranks of
union-find representatives) can differ — callers only use labels as ids.

`segment_points` is the same over-segmentation for a coloured point cloud that has no mesh: the edge
set is the symmetrised k-NN table of the cloud (`knn_edges`, csrc/felz_points.hip) instead of the triangles' sides; the
weights (`point_edge_weights`), the sort and the merge are the mesh path's.  The reference has no such function: it
reconstructs a mesh first (pseudo_masks/datasets/preprocess/stanford.py:80-135)."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import check, lib, require_device


def edge_weights(vertices: torch.Tensor, faces: torch.Tensor, colors: torch.Tensor):
    """Device part: -> (edge_a i32[3F], edge_b i32[3F], weights f32[3F], normals f32[V,3]), edges in face order."""
    require_device()
    ops._chk(vertices, torch.float32, "vertices")
    ops._chk(colors, torch.float32, "colors")
    ops._chk(faces, torch.int32, "faces")
    V, F = vertices.shape[0], faces.shape[0]
    if F > 0:
        # the device kernels dereference the indices: reject a malformed mesh BEFORE the first launch (one small
        # reduction + read-back; the module's call ends in a host merge anyway)
        lo, hi = torch.aminmax(faces)
        if int(lo) < 0 or int(hi) >= V:
            raise RuntimeError(f"felzenszwalb_cpp: face index out of range [0, {V}) (min {int(lo)}, max {int(hi)})")
    dev = vertices.device
    st = ops._stream
    fn = torch.empty((F, 3), dtype=torch.float32, device=dev)
    check(lib.usc_felz_face_normals(vertices.data_ptr(), faces.data_ptr(), F, fn.data_ptr(), st()), "usc_felz_face_normals")
    csr = ops.segment_csr(faces.reshape(-1).to(torch.int64).contiguous(), V)     # stable: faces stay in face order
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    check(lib.usc_felz_vertex_normals(fn.data_ptr(), csr.order.data_ptr(), csr.seg_off.data_ptr(), V,
                                      normals.data_ptr(), st()), "usc_felz_vertex_normals")
    ea = torch.empty(3 * F, dtype=torch.int32, device=dev)
    eb = torch.empty(3 * F, dtype=torch.int32, device=dev)
    w = torch.empty(3 * F, dtype=torch.float32, device=dev)
    check(lib.usc_felz_edge_weights(vertices.data_ptr(), colors.data_ptr(), normals.data_ptr(), faces.data_ptr(), F,
                                    ea.data_ptr(), eb.data_ptr(), w.data_ptr(), st()), "usc_felz_edge_weights")
    return ea, eb, w, normals


def merge_host(edge_a: np.ndarray, edge_b: np.ndarray, weights: np.ndarray, n_vertices: int, kthr: float,
               seg_min_verts: int) -> np.ndarray:
    """The sequential merge loops over edges ALREADY sorted by weight (host arrays) -> representative per vertex."""
    a = np.ascontiguousarray(edge_a, np.int32)
    b = np.ascontiguousarray(edge_b, np.int32)
    w = np.ascontiguousarray(weights, np.float32)
    comps = np.empty(n_vertices, np.int32)
    check(lib.usc_felz_merge_host(a.ctypes.data, b.ctypes.data, w.ctypes.data, a.shape[0], int(n_vertices), float(kthr),
                                  int(seg_min_verts), comps.ctypes.data), "usc_felz_merge_host")
    return comps


def relabel(comps: np.ndarray, edge_a: np.ndarray, edge_b: np.ndarray):
    """The wrapper's output convention (segmentator.cpp:200-240): labels = rank of the representative, connectivity =
    sorted set of directed (segment of a, segment of b) pairs over all edges with different segments."""
    _, labels = np.unique(comps, return_inverse=True)
    labels = labels.reshape(-1).astype(np.int32)
    s1, s2 = labels[edge_a], labels[edge_b]
    keep = s1 != s2
    if not keep.any():
        return labels, np.zeros((0, 2), np.int32)
    return labels, np.unique(np.stack([s1[keep], s2[keep]], 1), axis=0).astype(np.int32)


def segment_mesh(vertices, faces, colors, kthr: float = 0.005, segMinVerts: int = 20, device="cuda"):
    dev = torch.device(device)
    to = lambda x, dt: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(dev, dt).contiguous()
    v, c, f = to(vertices, torch.float32), to(colors, torch.float32), to(faces, torch.int32)
    ea, eb, w, _ = edge_weights(v, f, c)
    order = torch.sort(w, stable=True).indices            # equal weights keep face order
    host = torch.stack([ea[order].view(torch.float32), eb[order].view(torch.float32), w[order]]).cpu().numpy()   # one D2H
    sa, sb, sw = host[0].view(np.int32), host[1].view(np.int32), host[2]
    comps = merge_host(sa, sb, sw, v.shape[0], kthr, segMinVerts)
    return relabel(comps, sa, sb)


# ------------------------------------------------------------------------------------------------ point clouds (no mesh)
def knn_edges(idx: torch.Tensor, count: torch.Tensor, check_range: bool = True):
    """The undirected, deduplicated edge list of a k-NN table (usc_felz_knn_edges) -> (edge_a i32[E], edge_b i32[E]).

    idx i32[N,k], count i32[N] as `ops.knn_hybrid(points, points, k, radius)` writes them.  For row i ascending and
    position p < count[i] ascending, j = idx[i,p] != i gives the edge (i, j) iff i < j, or i > j and i is not in
    idx[j, :count[j]]: every pair of either list once, in (i, p) order.  The first count[i] entries of a row must be
    distinct and lie in [0, N); `check_range` tests the range (and 0 <= count <= k) with one reduction and one
    read-back before the first launch — a caller that made the table with `ops.knn_hybrid` passes False.
    The library writes into worst-case N*k buffers and leaves the total on the device; it is read back once here."""
    require_device()
    ops._chk(idx, torch.int32, "idx")
    ops._chk(count, torch.int32, "count")
    if idx.dim() != 2 or count.shape != (idx.shape[0],):
        raise RuntimeError("knn_edges: idx must be [N,k] and count [N]")
    n, k = idx.shape
    if not 1 <= k <= 64:
        raise RuntimeError(f"knn_edges: k must be 1 .. 64, got {k}")
    dev = idx.device
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    if check_range:
        used = torch.arange(k, device=dev, dtype=torch.int32)[None, :] < count[:, None]
        bad = (((idx < 0) | (idx >= n)) & used).any() | (count < 0).any() | (count > k).any()
        if bool(bad):
            raise RuntimeError(f"knn_edges: a used entry of idx lies outside [0, {n}) or a count outside [0, {k}]")
    nbytes = lib.usc_felz_knn_edges_ws_bytes(n)
    if nbytes < 0:
        check(-1, "usc_felz_knn_edges_ws_bytes")
    ws = ops._ws(nbytes, dev)
    ea = torch.empty(n * k, dtype=torch.int32, device=dev)
    eb = torch.empty(n * k, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    check(lib.usc_felz_knn_edges(idx.data_ptr(), count.data_ptr(), n, k, ea.data_ptr(), eb.data_ptr(), total.data_ptr(),
                                 ws.data_ptr(), ws.numel(), ops._stream()), "usc_felz_knn_edges")
    e = int(total.item())
    return ea[:e], eb[:e]


def point_edge_weights(points: torch.Tensor, colors: torch.Tensor, normals: torch.Tensor, edge_a: torch.Tensor,
                       edge_b: torch.Tensor, oriented: bool = True) -> torch.Tensor:
    """Felzenszwalb weights f32[E] of an explicit edge list (usc_felz_point_edge_weights).  oriented=True: the mesh
    kernel's arithmetic, bit for bit.  oriented=False, for estimated normals whose sign is arbitrary:
    normal_dist = 1 - |n_a . n_b| and no convexity squaring.  Coincident endpoints give a finite weight."""
    require_device()
    for t, name in ((points, "points"), (colors, "colors"), (normals, "normals")):
        ops._chk(t, torch.float32, name)
        if t.dim() != 2 or t.shape != (points.shape[0], 3):
            raise RuntimeError(f"point_edge_weights: {name} must be [{points.shape[0]},3], got {list(t.shape)}")
    ops._chk(edge_a, torch.int32, "edge_a")
    ops._chk(edge_b, torch.int32, "edge_b")
    if edge_a.dim() != 1 or edge_a.shape != edge_b.shape:
        raise RuntimeError("point_edge_weights: edge_a and edge_b must be [E]")
    w = torch.empty(edge_a.shape[0], dtype=torch.float32, device=points.device)
    check(lib.usc_felz_point_edge_weights(points.data_ptr(), colors.data_ptr(), normals.data_ptr(), points.shape[0],
                                          edge_a.data_ptr(), edge_b.data_ptr(), edge_a.shape[0], int(bool(oriented)),
                                          w.data_ptr(), ops._stream()), "usc_felz_point_edge_weights")
    return w


def _graph_args(k, radius):
    k, radius = int(k), float(radius)
    if not 0 <= k <= 63:
        raise ValueError(f"segment_points: k must be 0 .. 63 (the search asks for k + 1 <= 64 candidates), got {k}")
    if not (radius > 0 and np.isfinite(radius)):
        raise ValueError(f"segment_points: radius must be a positive finite number, got {radius!r}")
    return k, radius


def point_graph(points, colors, normals=None, k: int = 8, radius: float = 0.1, device="cuda", oriented=None):
    """The sorted graph of `segment_points`, which several segMinVerts levels share -> (edge_a i32[E], edge_b i32[E],
    weights f32[E]) as host arrays in non-decreasing weight order, equal weights in (i, p) order.  One k-NN search, one
    edge list, one weight launch, one stable device sort, one device-to-host copy.
    oriented: None means "normals were given"; a caller that estimated the normals itself passes them with False."""
    k, radius = _graph_args(k, radius)
    pts = np.asarray(points) if not isinstance(points, torch.Tensor) else points
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError(f"segment_points: points must be [N,3] with N >= 1, got {list(pts.shape)}")
    for x, name in ((colors, "colors"), (normals, "normals")):
        if x is not None and tuple(x.shape) != tuple(pts.shape):
            raise ValueError(f"segment_points: {name} must be {list(pts.shape)}, got {list(x.shape)}")
    dev = torch.device(device)
    to = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(dev, torch.float32).contiguous()
    p, c = to(points), to(colors)
    idx, count = ops.knn_hybrid(p, p, k + 1, radius)
    ea, eb = knn_edges(idx, count, check_range=False)
    n = ops.estimate_normals(p) if normals is None else to(normals)
    w = point_edge_weights(p, c, n, ea, eb, oriented=normals is not None if oriented is None else bool(oriented))
    order = torch.sort(w, stable=True).indices            # equal weights keep (i, p) order
    host = torch.stack([ea[order].view(torch.float32), eb[order].view(torch.float32), w[order]]).cpu().numpy()   # one D2H
    return host[0].view(np.int32), host[1].view(np.int32), host[2]


def relabel_symmetric(comps: np.ndarray, edge_a: np.ndarray, edge_b: np.ndarray):
    """`relabel` for an edge list that stores every undirected edge ONCE: labels as there, connectivity = the sorted set
    of (s(a), s(b)) and (s(b), s(a)) over the edges with different segments — the symmetric closure, because
    pseudo_masks/ncut.py `neighbour_sets` reads the pairs as directed."""
    labels, conn = relabel(comps, edge_a, edge_b)
    if conn.shape[0]:
        conn = np.unique(np.concatenate([conn, conn[:, ::-1]]), axis=0).astype(np.int32)
    return labels, conn


def segment_points(points, colors, normals=None, k: int = 8, radius: float = 0.1, kthr: float = 0.005,
                   segMinVerts: int = 20, device="cuda"):
    """Over-segmentation of a coloured point cloud without a mesh -> (labels i32[N] 0..S-1, connectivity i32[P,2]).

    points f32[N,3], colors f32[N,3] (in [0, 1], the scale `segment_mesh` is given for ScanNet), normals f32[N,3] or
    None.  The graph joins every point with its k nearest neighbours strictly inside `radius`
    (`ops.knn_hybrid(points, points, k + 1, radius)`: the point is one of its own candidates), each undirected pair once
    (`knn_edges`).  Given normals are taken as oriented and weighted as the mesh's are; normals=None estimates them
    (`ops.estimate_normals(points)`), whose sign is arbitrary, and weights with `oriented=False`.  Then the mesh path's
    stable device sort, one device-to-host copy, `merge_host` and `relabel`'s numbering; the connectivity is the
    symmetric closure (`relabel_symmetric`).
    UNMEASURED DEFAULTS: k=8 and radius=0.1 are a starting point nobody has measured on real scans;
    the radius wants to be a few point spacings, k near the valence of a mesh vertex."""
    sa, sb, sw = point_graph(points, colors, normals, k, radius, device)
    comps = merge_host(sa, sb, sw, int(points.shape[0]), kthr, segMinVerts)
    return relabel_symmetric(comps, sa, sb)
