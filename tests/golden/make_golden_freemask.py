#!/usr/bin/env python
"""Golden-vector generator for the FreeMask pipeline — runs ONLY where /root/reference exists (like make_golden.py,
whose stubs it uses).  Imports the reference's own `utils.freemask_utils.cosine_sim` and `utils.pc_utils.matrix_nms`
in place and drives them in the order of pseudo_masks/freemask_main.py:242-417 (voxel mode) on a planted scene; stores
the inputs and the reference's survivors in tests/golden/freemask.npz.  Nothing of the reference is copied; the
fixture is data.

    python tests/golden/make_golden_freemask.py

The planted scene: K = 1536 keys on a 16 x 16 x 6 grid (tensor stride 2), C = 96 = 6 blocks of 16 channels, one block
per feature cluster.  Cluster 5 is the "whole room" (the floor layer z = 0 and the walls x = 15, y >= 12: full x / y
extent, the extent filter must drop it); clusters 0-4 are objects (x // 3, y < 12, z >= 1: 2/15 and 11/15 of the scene).
82 keys (5.3 %) are all zero; of the other keys of every cluster exactly half are "core" (ones on the first 8 channels
of the block), half "halo" (ones on all 16: cosine 1/sqrt(2) to the core), each times a random magnitude.  Query i
(Q = 384, cluster i % 6, rows shuffled) is cos(t_i) core + sin(t_i) (halo - core) with t_i = (i + 1) / 385 * pi / 8, so
its mask is its cluster, and its maskness 1/2 + (1 + tan t_i) / (2 sqrt 2) is the same strictly increasing function of
t_i in every cluster: 384 distinct values at least 3.6e-4 apart.  Masks of one cluster are identical (IoU 1), masks of
different clusters disjoint (IoU 0).

The generator asserts the margins that make the decisions independent of f32 summation order, and fails otherwise:
no two candidate maskness values closer than 1e-4; no compared pair with |inter/union - 0.5| < 0.02; no survivor's
maskness within 0.01 of 0.6.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

K_GRID, C, Q = (16, 16, 6), 96, 384
PARAMS = dict(hard_mask_threshold=0.35, min_mask_points=10, instance_to_scene_max_ratio=0.8, nms_thr=0.5,
              max_instance_num=50, nms_maskness_threshold=0.6)


def build_inputs():
    rng = np.random.default_rng(77)
    gx, gy, gz = np.meshgrid(*[np.arange(n) for n in K_GRID], indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1)
    grid = grid[rng.permutation(len(grid))]
    room = (grid[:, 2] == 0) | (grid[:, 0] == 15) | (grid[:, 1] >= 12)
    cluster = np.where(room, 5, grid[:, 0] // 3)
    fk = np.zeros((len(grid), C), np.float32)
    n_zero = 0
    for j in range(6):
        rows = np.nonzero(cluster == j)[0]
        nz = 32 if j == 5 else 10                             # zero keys of this cluster; the rest splits evenly
        assert (len(rows) - nz) % 2 == 0
        n_zero += nz
        live = rows[nz:]
        fk[live[0::2], 16 * j:16 * j + 8] = 1.0              # core
        fk[live[1::2], 16 * j:16 * j + 16] = 1.0             # halo
    fk *= rng.uniform(0.5, 2.0, (len(grid), 1)).astype(np.float32)
    t = (np.arange(Q) + 1) / (Q + 1) * np.pi / 8
    fq = np.zeros((Q, C), np.float32)
    for i in range(Q):
        j = i % 6
        fq[i, 16 * j:16 * j + 8] = np.cos(t[i])
        fq[i, 16 * j + 8:16 * j + 16] = np.sin(t[i])
    perm = rng.permutation(Q)
    fq, q_cluster = fq[perm], (np.arange(Q) % 6)[perm]
    fq *= rng.uniform(0.5, 2.0, (Q, 1)).astype(np.float32)
    coords = (grid * 2).astype(np.int32)                     # tensor stride 2
    return fk, fq, coords, cluster, q_cluster, n_zero


def run_reference(cosine_sim, matrix_nms, fk, fq, coords, scene_extents):
    """freemask_main.py:242-417 with segment_ids == [] (voxel mode), line for line."""
    P = PARAMS
    key_feats, queries = torch.from_numpy(fk), torch.from_numpy(fq)
    lr_coords = coords
    soft_masks = cosine_sim(key_feats, queries)                                              # :242
    soft_masks[:, torch.all(key_feats == 0, dim=-1)] = 0.                                    # :266
    masks = soft_masks >= P["hard_mask_threshold"]
    sum_masks = masks.sum(1)
    keep = sum_masks > P["min_mask_points"]                                                  # :271
    assert keep.sum() > 0
    cand_index = torch.nonzero(keep).flatten()
    masks, soft_masks, sum_masks = masks[keep], soft_masks[keep], sum_masks[keep]
    maskness = (soft_masks * masks.float()).sum(1) / sum_masks                               # :353
    srt = torch.sort(maskness).values
    assert float((srt[1:] - srt[:-1]).min()) >= 1e-4, "two candidate maskness values closer than 1e-4"
    sort_inds = torch.argsort(maskness, descending=True)
    maskness, soft_masks, cand_index = maskness[sort_inds], soft_masks[sort_inds], cand_index[sort_inds]
    masks = (soft_masks >= P["hard_mask_threshold"]).bool()                                  # :372
    filtered_masks = []                                                                      # :375-395
    for mask_id in range(len(masks)):
        if torch.all(~masks[mask_id]):
            continue
        inst_coords = lr_coords[masks[mask_id].numpy()]
        inst_extent = inst_coords.max(0) - inst_coords.min(0)
        extent_ratios = inst_extent / scene_extents
        if np.any(extent_ratios[:2] > P["instance_to_scene_max_ratio"]):
            continue
        filtered_masks += [mask_id]
    assert filtered_masks != []
    n_dropped_by_extent = len(masks) - len(filtered_masks)
    masks, soft_masks, maskness = masks[filtered_masks], soft_masks[filtered_masks], maskness[filtered_masks]
    cand_index = cand_index[filtered_masks]
    sum_masks = masks.sum(1)
    # the margins of every pair the greedy loop compares (recomputed here; the loop itself is the reference's)
    m = masks.numpy()
    alive = np.ones(len(m), bool)
    for i in range(len(m)):
        if not alive[i]:
            continue
        for j in range(i + 1, len(m)):
            if not alive[j]:
                continue
            inter = int((m[i] & m[j]).sum())
            union = int(m[i].sum()) + int(m[j].sum()) - inter
            assert union > 0 and abs(inter / union - 0.5) >= 0.02, "a compared pair within 0.02 of IoU 1/2"
            if inter / union > P["nms_thr"]:
                alive[j] = False
    maskness = matrix_nms(maskness * 0, masks, sum_masks, maskness, sigma=2, kernel='mask',
                          nms_thr=P["nms_thr"])                                              # :398
    assert np.array_equal(maskness.numpy() > 0, alive)
    sort_inds = torch.argsort(maskness, descending=True)
    if len(sort_inds) > P["max_instance_num"]:
        sort_inds = sort_inds[:P["max_instance_num"]]
    maskness, soft_masks, cand_index = maskness[sort_inds], soft_masks[sort_inds], cand_index[sort_inds]
    keep = maskness > P["nms_maskness_threshold"]                                            # :412
    assert keep.sum() > 0
    assert float((maskness[keep] - P["nms_maskness_threshold"]).abs().min()) >= 0.01
    assert float((maskness[~keep] - P["nms_maskness_threshold"]).abs().min()) >= 0.01 if (~keep).any() else True
    return soft_masks[keep].numpy(), maskness[keep].numpy(), cand_index[keep].numpy(), n_dropped_by_extent


def main():
    make_golden.stub("open3d", "hdbscan", "MinkowskiEngine", "plyfile", "pandas", "matplotlib", "matplotlib.pyplot",
                     "cv2")
    sys.path.insert(0, make_golden.REF)
    sys.path.insert(0, os.path.join(make_golden.REF, "pseudo_masks"))
    from utils.freemask_utils import cosine_sim
    from utils.pc_utils import matrix_nms

    fk, fq, coords, cluster, q_cluster, n_zero = build_inputs()
    scene_extents = (coords.max(0) - coords.min(0)).astype(np.int64)
    soft, maskness, qidx, n_dropped = run_reference(cosine_sim, matrix_nms, fk, fq, coords, scene_extents)
    assert n_zero == int(np.all(fk == 0, 1).sum()) and 0.04 < n_zero / len(fk) < 0.06
    assert n_dropped == 64, "every whole-room mask, and only those, fails the extent filter"
    assert sorted(q_cluster[qidx].tolist()) == [0, 1, 2, 3, 4], "one survivor per object cluster, none for the room"
    path = os.path.join(HERE, "freemask.npz")
    np.savez_compressed(path, key_feats=fk, query_feats=fq, key_coords=coords,
                        scene_extent=scene_extents.astype(np.float32), key_cluster=cluster.astype(np.int8),
                        query_cluster=q_cluster.astype(np.int8), soft_masks=soft, maskness=maskness,
                        query_index=qidx.astype(np.int64),
                        **{f"param_{k}": np.float64(v) for k, v in PARAMS.items()})
    print("survivors", qidx.tolist(), "maskness", maskness.tolist())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
