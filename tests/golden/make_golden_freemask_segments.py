#!/usr/bin/env python
"""Golden-vector generator for FreeMask SEGMENT mode — runs ONLY where /root/reference exists (like
make_golden_freemask.py, whose stubs it shares).  Imports the reference's own `utils.freemask_utils.cosine_sim`,
`utils.pc_utils.matrix_nms` and `utils.point_cloud_utils.separate_segments` (the scan of freemask_main.py:288-327 as a
function) in place and calls them in the order of the script's segment mode on a planted scene; the steps between
them (segment means, neighbour sets, parts to rows, remap, extent filter) are this project's own array code, written
from the mode's description.  Stores the inputs and the survivors in tests/golden/freemask_segments.npz; the fixture
is data.

    python tests/golden/make_golden_freemask_segments.py

The planted scene.  Key voxels on a 24 x 20 x 6 grid at tensor stride 2 (coordinates = 2 * grid), C = 16 = 6 feature
clusters x 2 channels + 4 unused; a segment's feature is (cos t, sin t) on its cluster's channel pair (t random in
[0, 50 deg] for the room and the objects: cos 50 deg > 0.35, other clusters are orthogonal), a voxel's
feature its segment's times a magnitude in [0.5, 2); about 5 % of the voxels are all zero.  Segments are columns over
cells of 2 x 2 voxels, of different heights (4 to 20 voxels):
* the "room" (cluster 5): the whole floor z = 0 in 30 patches of 4 x 4 voxels, one connected part of full x / y extent:
  the extent filter must drop all of its rows;
* objects 0-3: each a group A of 2 x 3 cells and a group B of 2 x 2 cells that do not touch: every query gives two rows;
  object 0 has a third group C of 2 cells: a part of <= 3 segments, dropped;
* a cell Z between A and B of object 1 with only zero voxels: dropped as a segment, still named by connectivity pairs
  (it would bridge A and B);
* the "fan" (cluster 4), one connected row of cells: G0 (6 cells of 4 voxels, t ~ 0), G30 (1 cell of 4 voxels,
  t ~ 30 deg), G90 (2 cells of 20 voxels, t ~ 90 deg).  cos 90 deg < 0.35 <= cos 60 deg, so the masks are P = G0 + G30
  (queries of G0), Q = all nine (the query of G30) and T = G30 + G90 (queries of G90, 3 segments: dropped).  P against Q
  is IoU 7/9 by segments (suppressed) and 28/68 by voxels (kept): Q survives only with voxel counts.
Segment ids are scattered in [3, 9000); the connectivity lists every touching pair of segments in both directions
(objects touch the floor, which is outside their masks).  The input level (stride 1) lists for every key voxel a random
non-empty subset of its 8 children, each carrying the key's feature; one child carries the key's id, the others
smaller ids, so max pooling gives the key ids back.

The generator asserts the margins that make the decisions independent of f32 summation order, and fails otherwise:
no two rows' maskness closer than 4e-5 (about 120 rows share [0.80, 0.99]; an f32 mean of at most 30 values in [0, 1]
is off by at most 30 * 2^-24 = 2e-6 plus the soft values' own error of the same order, and the tests compare maskness
within 1e-5: the gap is four times that bound; the seed is the first one that gives it); no compared pair with |inter/union - 0.5| < 0.02, by voxel counts;
no row's maskness within 0.01 of 0.6 after the NMS; no soft value of a candidate within 0.01 of 0.35; the reference's
scan equal to the true undirected components for every candidate (deviation (d) not in play); at least one compared
pair on different sides of nms_thr by segment-count IoU and by voxel-count IoU.

It also records a hand-made graph (`bridge_*`) on which the reference's scan leaves two connected blobs apart: the
segment inserted last touches three earlier blobs, and the blob that slides into the popped blob's place is skipped.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402

GRID, C = (24, 20, 6), 16
PARAMS = dict(hard_mask_threshold=0.35, min_mask_segments=2, min_part_segments=3, instance_to_scene_max_ratio=0.8,
              nms_thr=0.5, max_instance_num=50, nms_maskness_threshold=0.6)
ROOM, FAN = 5, 4


def build_inputs(seed):
    rng = np.random.default_rng(seed)
    seg_of = -np.ones(GRID, np.int64)                       # provisional segment number per grid voxel, -1 = empty
    cluster, angle, zero_seg = [], [], []

    def add(cells, height, cl, t, zero=False):
        for cx, cy in cells:
            n = len(cluster)
            seg_of[2 * cx:2 * cx + 2, 2 * cy:2 * cy + 2, 1:1 + height] = n
            cluster.append(cl)
            angle.append(t())
            zero_seg.append(zero)

    for px in range(6):                                     # the floor
        for py in range(5):
            seg_of[4 * px:4 * px + 4, 4 * py:4 * py + 4, 0] = len(cluster)
            cluster.append(ROOM)
            angle.append(rng.uniform(0, np.deg2rad(50)))
            zero_seg.append(False)
    obj_t = lambda: rng.uniform(0, np.deg2rad(50))          # noqa: E731
    for j, cx0 in enumerate((0, 3, 6, 9)):
        add([(cx0 + i, cy) for i in range(2) for cy in range(3)], 5, j, obj_t)               # A
        cy0 = (5, 4, 6, 6)[j]
        add([(cx0 + i, cy0 + k) for i in range(2) for k in range(2)], 3, j, obj_t)           # B
    add([(0, 8), (0, 9)], 2, 0, obj_t)                                                       # C of object 0
    add([(3, 3)], 2, 1, obj_t, zero=True)                                                    # Z
    jitter = iter(np.deg2rad((rng.permutation(9) - 4.0) / 2))
    add([(cx, 9) for cx in range(2, 8)], 1, FAN, lambda: next(jitter))                       # G0
    add([(8, 9)], 1, FAN, lambda: np.deg2rad(30) + next(jitter))                             # G30
    add([(9, 9), (10, 9)], 5, FAN, lambda: np.deg2rad(90) + next(jitter))                    # G90
    n_seg = len(cluster)
    seg_id = np.sort(rng.choice(np.arange(3, 9000), n_seg, replace=False))[rng.permutation(n_seg)]

    grid = np.argwhere(seg_of >= 0)
    grid = grid[rng.permutation(len(grid))]
    num = seg_of[tuple(grid.T)]
    key_ids = seg_id[num]
    direction = np.zeros((n_seg, C))
    for n in range(n_seg):
        direction[n, 2 * cluster[n]], direction[n, 2 * cluster[n] + 1] = np.cos(angle[n]), np.sin(angle[n])
    fk = direction[num] * rng.uniform(0.5, 2.0, (len(grid), 1))
    fk[rng.random(len(grid)) < 0.05] = 0.0
    fk[np.asarray(zero_seg)[num]] = 0.0
    fk = fk.astype(np.float32)
    for n in range(n_seg):
        assert zero_seg[n] or np.any(fk[num == n] != 0), "a live segment lost all its voxels to the zeroing"
    # connectivity: every pair of 6-neighbouring voxels of different segments, both directions
    pairs = set()
    for axis in range(3):
        a = np.moveaxis(seg_of, axis, 0)
        u, v = a[:-1].ravel(), a[1:].ravel()
        for x, y in zip(u[(u >= 0) & (v >= 0) & (u != v)], v[(u >= 0) & (v >= 0) & (u != v)]):
            pairs.add((int(seg_id[x]), int(seg_id[y])))
            pairs.add((int(seg_id[y]), int(seg_id[x])))
    conn = np.array(sorted(pairs), np.int64)
    conn = conn[rng.permutation(len(conn))]
    coords = (grid * 2).astype(np.int32)
    # the input level
    in_coords, in_parent, in_ids = [], [], []
    offsets = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)])
    for v in range(len(grid)):
        kids = offsets[rng.permutation(8)[:rng.integers(1, 9)]]
        carrier = rng.integers(len(kids))
        for c, o in enumerate(kids):
            in_coords.append(coords[v] + o)
            in_parent.append(v)
            in_ids.append(key_ids[v] if c == carrier else rng.integers(0, key_ids[v] + 1))
    order = rng.permutation(len(in_coords))
    meta = dict(cluster=np.asarray(cluster)[num].astype(np.int8), n_seg=n_seg, zero_ids=seg_id[np.asarray(zero_seg)])
    return (fk, coords, key_ids, conn, np.asarray(in_coords, np.int32)[order], np.asarray(in_parent, np.int64)[order],
            np.asarray(in_ids, np.int64)[order], meta)


def true_components(ids_in_mask, conn):
    """Undirected components over the ids of one mask -> sorted list of sorted id lists."""
    ids = [int(s) for s in ids_in_mask]
    parent = {s: s for s in ids}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in conn:
        a, b = int(a), int(b)
        if a in parent and b in parent and a != b:
            parent[find(a)] = find(b)
    groups = {}
    for s in ids:
        groups.setdefault(find(s), []).append(s)
    return sorted(sorted(g) for g in groups.values())


def run_reference(cosine_sim, matrix_nms, separate_segments, fk, key_coords, key_ids, conn, scene_extents):
    """The reference's three functions, called in the order its segment mode calls them.  The glue between them is
    written from the description of that mode with array operations, in f32 like the
    script: segment means by one scatter-add, parts scattered into rows through a boolean [parts, S] table, the remap as
    one gather, the extent filter as two masked reductions."""
    P = PARAMS
    thr = P["hard_mask_threshold"]
    # step 2: mean of the seen (not all-zero) key rows per segment, all-zero segments dropped, idx(v)
    ids_all, inv = np.unique(key_ids, return_inverse=True)
    inv = inv.reshape(-1)
    seen = np.any(fk != 0, axis=1)
    sums = torch.zeros((len(ids_all), fk.shape[1])).index_add_(0, torch.from_numpy(inv[seen]), torch.from_numpy(fk[seen]))
    n_seen = np.bincount(inv[seen], minlength=len(ids_all))
    means = sums / torch.from_numpy(np.maximum(n_seen, 1)).float()[:, None]
    live = np.any(means.numpy() != 0, axis=1)
    ids, seg_feats = ids_all[live], means[torch.from_numpy(live)]
    S = len(ids)
    idx = np.where(live, np.cumsum(live) - 1, -1)[inv]
    # the directed neighbour sets the scan reads (out-neighbours only, as the script builds them)
    out_nbrs = {int(s): set() for s in ids}
    for a, b in conn.tolist():
        if a in out_nbrs:
            out_nbrs[a].add(b)
    # step 3: cosine masks of the segments against themselves
    soft = cosine_sim(seg_feats.clone(), seg_feats.clone())
    assert not bool((seg_feats == 0).all(1).any())               # no all-zero key column is left to clear
    member = (soft >= thr).numpy()
    cand = np.flatnonzero(member.sum(1) > P["min_mask_segments"])
    assert len(cand) > 0
    assert float((soft[torch.from_numpy(cand)] - thr).abs().min()) >= 0.01, "a candidate's soft value near 0.35"
    # step 4: the reference's scan per candidate -> one row per blob
    owner, cols = [], []
    for q in cand:
        blobs = separate_segments(member[q], ids, out_nbrs)
        blobs = [sorted(int(s) for s in blob) for blob in blobs]
        assert sorted(blobs) == true_components(ids[member[q]], conn), "the reference's scan differs from the true components"
        for blob in blobs:
            owner.append(q)
            cols.append(np.searchsorted(ids, blob))
    in_part = np.zeros((len(cols), S), bool)
    for r, c in enumerate(cols):
        in_part[r, c] = True
    owner = np.asarray(owner)
    root = np.array([ids[c.min()] for c in cols], np.int64)
    rows = torch.where(torch.from_numpy(in_part), soft[torch.from_numpy(owner)], torch.zeros(()))
    n_segs = in_part.sum(1)
    big = n_segs > P["min_part_segments"]
    n_small_parts = int((~big).sum())
    rows, in_part, owner, root, n_segs = rows[torch.from_numpy(big)], in_part[big], owner[big], root[big], n_segs[big]
    maskness = rows.sum(1) / torch.from_numpy(n_segs)            # rows are zero outside the part, >= thr inside
    gaps = np.diff(np.sort(maskness.numpy()))
    assert gaps.min() >= 4e-5, "two candidate maskness values closer than 4e-5"
    by = torch.argsort(maskness, descending=True)
    maskness, rows = maskness[by], rows[by]
    in_part, owner, root = in_part[by.numpy()], owner[by.numpy()], root[by.numpy()]
    # step 5: remap by one gather (column S is the zero column of voxels without a live segment), extent on x and y
    padded = torch.cat([rows, torch.zeros((len(rows), 1))], 1)
    vox = padded[:, torch.from_numpy(np.where(idx >= 0, idx, S))]
    vmask = (vox >= thr).numpy()
    assert vmask.any(1).all()
    xy = key_coords[:, :2].astype(np.int64)
    far = np.iinfo(np.int64).max
    hi = np.where(vmask[:, :, None], xy[None], -far).max(1)
    lo = np.where(vmask[:, :, None], xy[None], far).min(1)
    fits = ~np.any((hi - lo) / scene_extents[:2] > P["instance_to_scene_max_ratio"], axis=1)
    assert fits.any()
    n_dropped_by_extent = int((~fits).sum())
    maskness, vox = maskness[torch.from_numpy(fits)], vox[torch.from_numpy(fits)]
    vmask, in_part, owner, root = vmask[fits], in_part[fits], owner[fits], root[fits]
    # margins of every pair the greedy loop compares, and the pairs the two kinds of IoU decide differently
    alive = np.ones(len(vmask), bool)
    n_differ = 0
    for i in range(len(vmask)):
        if not alive[i]:
            continue
        for j in range(i + 1, len(vmask)):
            if not alive[j]:
                continue
            inter = int((vmask[i] & vmask[j]).sum())
            union = int(vmask[i].sum()) + int(vmask[j].sum()) - inter
            assert union > 0 and abs(inter / union - 0.5) >= 0.02, "a compared pair within 0.02 of IoU 1/2"
            s_inter = int((in_part[i] & in_part[j]).sum())
            s_iou = s_inter / (int(in_part[i].sum()) + int(in_part[j].sum()) - s_inter)
            assert abs(s_iou - 0.5) >= 0.02
            n_differ += (s_iou > P["nms_thr"]) != (inter / union > P["nms_thr"])
            if inter / union > P["nms_thr"]:
                alive[j] = False
    assert n_differ >= 1, "no compared pair decided differently by segment counts and by voxel counts"
    # step 6: the reference's NMS on the voxel masks with their own voxel counts, then the two cuts
    vm = torch.from_numpy(vmask)
    maskness = matrix_nms(torch.zeros_like(maskness), vm, vm.sum(1), maskness, sigma=2, kernel='mask',
                          nms_thr=P["nms_thr"])
    assert np.array_equal(maskness.numpy() > 0, alive)
    by = torch.argsort(maskness, descending=True)[:P["max_instance_num"]]
    maskness, vox, owner, root = maskness[by], vox[by], owner[by.numpy()], root[by.numpy()]
    final = (maskness > P["nms_maskness_threshold"]).numpy()
    assert final.any()
    assert float((maskness - P["nms_maskness_threshold"]).abs().min()) >= 0.01
    stats = dict(n_dropped_segments=int((~live).sum()), n_small_parts=n_small_parts,
                 n_dropped_by_extent=n_dropped_by_extent, n_differ=n_differ, n_segments=S)
    return vox.numpy()[final], maskness.numpy()[final], ids[owner[final]], root[final], stats


def bridge_case(separate_segments):
    """Five segments; mask = all.  Ids 1, 2, 3 are pairwise unconnected and 5 (inserted last) touches all three: the
    scan merges blob {2} into {1}, pops it, steps over blob {3} that slid into its place, and leaves {3} apart although
    3 - 5 is a pair.  4 is isolated."""
    ids = np.array([1, 2, 3, 4, 5], np.int64)
    conn = np.array([[5, 1], [1, 5], [5, 2], [2, 5], [5, 3], [3, 5]], np.int64)
    cd = {int(s): set() for s in ids}
    for a, b in conn.tolist():
        cd[a].add(b)
    blobs = separate_segments(np.ones(5, bool), ids, cd)
    got = sorted(sorted(int(s) for s in b) for b in blobs)
    assert got != true_components(ids, conn), "the hand-made graph does not show the reference's skipped blob"
    label = -np.ones(5, np.int64)                            # the reference's blobs as labels (smallest id of the blob)
    for b in got:
        for s in b:
            label[np.searchsorted(ids, s)] = b[0]
    return ids, conn, label


def main():
    make_golden.stub("open3d", "hdbscan", "MinkowskiEngine", "plyfile", "pandas", "matplotlib", "matplotlib.pyplot",
                     "cv2")
    sys.path.insert(0, make_golden.REF)
    sys.path.insert(0, os.path.join(make_golden.REF, "pseudo_masks"))
    from utils.freemask_utils import cosine_sim
    from utils.pc_utils import matrix_nms
    from utils.point_cloud_utils import separate_segments

    import freemask_segment_ref as SR
    for seed in range(5000):        # the first seed whose rows' maskness values are well apart (asserted again below)
        fk, coords, key_ids, conn, in_coords, in_parent, in_ids, meta = build_inputs(seed)
        dbg = {}
        SR.freemask_segments_ref(fk, coords, key_ids, conn, coords.max(0) - coords.min(0), debug=dbg, **PARAMS)
        if np.diff(np.sort(dbg["maskness_sorted"])).min() >= 5e-5:
            break
    else:
        raise SystemExit("no seed gives maskness gaps of 5e-5")
    print("seed", seed)
    pooled_coords, pooled_ids = SR.maxpool_ids(in_coords, in_ids, 1)
    order = np.lexsort(coords.T[::-1])
    assert np.array_equal(pooled_coords, coords[order]) and np.array_equal(pooled_ids, key_ids[order])
    scene_extents = (coords.max(0) - coords.min(0)).astype(np.int64)
    soft, maskness, query, root, stats = run_reference(cosine_sim, matrix_nms, separate_segments, fk, coords, key_ids,
                                                       conn, scene_extents)
    print(stats)
    assert 65 <= stats["n_segments"] <= 200 and stats["n_dropped_segments"] == 1
    assert stats["n_small_parts"] >= 1 and stats["n_dropped_by_extent"] == 30
    assert all(np.any(conn == z) for z in meta["zero_ids"]), "the dropped segment must still be named by pairs"
    assert 0.03 < np.all(fk == 0, 1).mean() < 0.09
    b_ids, b_conn, b_label = bridge_case(separate_segments)
    path = os.path.join(HERE, "freemask_segments.npz")
    np.savez_compressed(path, key_feats=fk, key_coords=coords, key_segment_ids=key_ids, seg_connectivity=conn,
                        scene_extent=scene_extents.astype(np.float32), key_cluster=meta["cluster"],
                        in_coords=in_coords, in_parent=in_parent, in_segment_ids=in_ids,
                        soft_masks=soft, maskness=maskness, query_segment=query.astype(np.int64),
                        part_root=root.astype(np.int64), bridge_ids=b_ids, bridge_conn=b_conn,
                        bridge_reference_label=b_label,
                        **{f"param_{k}": np.float64(v) for k, v in PARAMS.items()})
    print("survivors (query, root)", list(zip(query.tolist(), root.tolist())), "maskness", maskness.tolist())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
