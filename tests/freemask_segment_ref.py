"""float64 numpy restatement of the FreeMask segment-mode pipeline (unscene3d_amd/pseudo_masks/freemask.py,
`freemask_segments`), written from its description, not from the device code.  It works at VOXEL level wherever the
reference does (remap, extent, NMS); `segment_level_quantities` gives the same numbers from the S-bit rows and the
per-segment tables, and the host tests show the two agree.

  1  ids per key voxel: max over the present children, per level (floor-divided coordinates)
  2  unique_segments = sorted unique ids; feature = mean of the not-all-zero key rows of the segment; all-zero segments
     dropped; idx(v) in [0, S) or -1
  3  a = cosine rows of the S segment features against themselves (freemask_ref.cosine_rows); mask = a >= threshold;
     candidates: more than min_mask_segments segments
  4  every candidate's mask is split into the connected components of the UNDIRECTED adjacency restricted to the mask
     (pairs naming an unknown / dropped id and self pairs ignored); one row per part, ordered by the part's smallest
     segment index; rows with more than min_part_segments segments stay; maskness = sum(soft) / segments; stable sort
  5  remap: voxel v carries row[idx(v)], 0 where idx(v) = -1; extent filter on voxel coordinates (x, y); none -> all stay
  6  greedy NMS on the voxel masks with voxel counts (freemask_ref.greedy_nms); stable sort; cuts
  7  soft rows f64[M, K], maskness, the query's segment id, the part's smallest segment id
"""
import numpy as np

import freemask_ref as FR


def maxpool_ids(coords, ids, steps=1, stride=1):
    """Floor-divide the coordinates `steps` times -> (coarse coords int64[P,3] multiples of the new stride, sorted
    lexicographically; ids int64[P] = max over the children)."""
    coords, ids = np.asarray(coords, np.int64), np.asarray(ids, np.int64)
    for _ in range(steps):
        stride *= 2
        parent = np.floor_divide(coords, stride) * stride
        coords, inv = np.unique(parent, axis=0, return_inverse=True)
        out = np.full(len(coords), np.iinfo(np.int64).min)
        np.maximum.at(out, inv.reshape(-1), ids)
        ids = out
    return coords, ids


def segment_features(fk, ids):
    """-> (seg_feats f64[S,C], unique_segments int64[S], idx int64[K] with -1 for voxels of dropped segments)."""
    fk, ids = np.asarray(fk, np.float64), np.asarray(ids, np.int64)
    uniq = np.unique(ids)
    nonzero = np.any(fk != 0, axis=1)
    feats = np.zeros((len(uniq), fk.shape[1]))
    for i, s in enumerate(uniq):
        rows = nonzero & (ids == s)
        if rows.any():
            feats[i] = fk[rows].mean(0)
    valid = np.any(feats != 0, axis=1)
    new_index = np.where(valid, np.cumsum(valid) - 1, -1)
    return feats[valid], uniq[valid], new_index[np.searchsorted(uniq, ids)]


def undirected_adjacency(conn, unique_segments):
    """-> list of S sets of segment INDICES: symmetric, no self loops, unknown ids ignored."""
    index = {int(s): i for i, s in enumerate(unique_segments)}
    adj = [set() for _ in unique_segments]
    for a, b in np.asarray(conn, np.int64).reshape(-1, 2):
        ia, ib = index.get(int(a)), index.get(int(b))
        if ia is None or ib is None or ia == ib:
            continue
        adj[ia].add(ib)
        adj[ib].add(ia)
    return adj


def components(mask, adj):
    """Union-find.  mask bool[S], adj list of sets -> label int64[S]: -1 outside the mask, else the smallest index of
    the connected component inside the mask."""
    mask = np.asarray(mask, bool)
    parent = np.arange(len(mask))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for s in np.nonzero(mask)[0]:
        for t in adj[s]:
            if mask[t]:
                a, b = find(s), find(t)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return np.array([find(s) if mask[s] else -1 for s in range(len(mask))], np.int64)


def split_rows(a, masks, cand, adj, min_part_segments=3):
    """-> (rows f64[R,S], query index int64[R], root int64[R]) in (query, root) order, small parts dropped."""
    rows, query, root = [], [], []
    for q in cand:
        label = components(masks[q], adj)
        for r in np.unique(label[label >= 0]):
            part = label == r
            if part.sum() > min_part_segments:
                rows.append(np.where(part, a[q], 0.0))
                query.append(q)
                root.append(r)
    S = a.shape[1]
    return np.array(rows).reshape(-1, S), np.array(query, np.int64), np.array(root, np.int64)


def remap(rows, idx):
    """f64[R,S] -> f64[R,K]: voxel v carries rows[:, idx[v]], 0 where idx[v] = -1."""
    padded = np.concatenate([rows, np.zeros((len(rows), 1))], 1)
    return padded[:, np.where(idx >= 0, idx, rows.shape[1])]


def segment_tables(idx, coords, S):
    """w int64[S], lo / hi int64[S,3] from the key voxels of every segment."""
    coords = np.asarray(coords, np.int64)
    w = np.zeros(S, np.int64)
    lo = np.full((S, 3), np.iinfo(np.int32).max, np.int64)
    hi = np.full((S, 3), np.iinfo(np.int32).min, np.int64)
    for s in range(S):
        rows = idx == s
        w[s] = rows.sum()
        if w[s]:
            lo[s], hi[s] = coords[rows].min(0), coords[rows].max(0)
    return w, lo, hi


def segment_level_quantities(seg_masks, w, lo, hi):
    """Voxel counts, boxes and pairwise voxel intersections of unions of whole segments from segment-level data only:
    -> (count int64[R], lo int64[R,3], hi int64[R,3], inter int64[R,R])."""
    seg_masks = np.asarray(seg_masks, bool)
    count = seg_masks.astype(np.int64) @ w
    big = np.iinfo(np.int32).max
    box_lo = np.array([lo[m].min(0) if m.any() else [big] * 3 for m in seg_masks], np.int64).reshape(-1, 3)
    box_hi = np.array([hi[m].max(0) if m.any() else [-big - 1] * 3 for m in seg_masks], np.int64).reshape(-1, 3)
    inter = (seg_masks.astype(np.int64) * w) @ seg_masks.astype(np.int64).T
    return count, box_lo, box_hi, inter


def freemask_segments_ref(fk, coords, ids, conn, scene_extent, hard_mask_threshold=0.35, min_mask_segments=2,
                          min_part_segments=3, instance_to_scene_max_ratio=0.8, nms_thr=0.5, max_instance_num=50,
                          nms_maskness_threshold=0.6, debug=None):
    """-> (soft rows f64[M,K], maskness f64[M], query segment id int64[M], part root segment id int64[M]).
    `debug` (a dict) receives the intermediate arrays."""
    coords = np.asarray(coords, np.int64)[:, -3:]
    K = len(coords)
    empty = (np.zeros((0, K)), np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64))
    seg_feats, uniq, idx = segment_features(fk, ids)
    S = len(uniq)
    if S == 0:
        return empty
    a, _, _, _ = FR.cosine_rows(seg_feats, seg_feats)
    masks = a >= hard_mask_threshold
    cand = np.nonzero(masks.sum(1) > min_mask_segments)[0]
    if len(cand) == 0:
        return empty
    adj = undirected_adjacency(conn, uniq)
    rows, query, root = split_rows(a, masks, cand, adj, min_part_segments)
    if len(rows) == 0:
        return empty
    seg_masks = rows >= hard_mask_threshold
    maskness = (rows * seg_masks).sum(1) / seg_masks.sum(1)
    by = np.argsort(-maskness, kind="stable")
    rows, query, root, maskness, seg_masks = rows[by], query[by], root[by], maskness[by], seg_masks[by]
    vox = remap(rows, idx)
    vmasks = vox >= hard_mask_threshold
    lo, hi = FR.mask_extent(vmasks, coords)
    ratios = (hi - lo)[:, :2] / np.asarray(scene_extent, np.float64)[:2]
    ok = ~np.any(ratios > instance_to_scene_max_ratio, axis=1)
    if debug is not None:
        debug.update(seg_feats=seg_feats, unique_segments=uniq, idx=idx, a=a, adj=adj, rows=rows, seg_masks=seg_masks,
                     voxel_masks=vmasks, extent_ok=ok, maskness_sorted=maskness, query=query, root=root)
    if ok.any():
        vox, vmasks, query, root, maskness = vox[ok], vmasks[ok], query[ok], root[ok], maskness[ok]
    keep = FR.greedy_nms(vmasks, vmasks.sum(1), nms_thr)
    maskness = np.where(keep, maskness, 0.0)
    by = np.argsort(-maskness, kind="stable")[:max_instance_num]
    vox, query, root, maskness = vox[by], query[by], root[by], maskness[by]
    sel = maskness > nms_maskness_threshold
    if not sel.any():
        return empty
    return vox[sel], maskness[sel], uniq[query[sel]], uniq[root[sel]]
