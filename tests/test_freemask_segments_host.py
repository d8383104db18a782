"""CPU: the float64 restatement tests/freemask_segment_ref.py reproduces the reference's own segment-mode run
(tests/golden/freemask_segments.npz, written by tests/golden/make_golden_freemask_segments.py from the reference's
cosine_sim, separate_segments and matrix_nms); the voxel-level quantities it works with equal the segment-level
formulas the device path uses; and on the recorded triple-bridge graph it gives the true components where the
reference's scan does not (deviation (d)); and the package's selection tail picks the restatement's survivors from
the restatement's split rows."""
import os

import numpy as np
import pytest

import freemask_ref as FR
import freemask_segment_ref as SR
import test_freemask_host as TH

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freemask_segments.npz")


def golden_params(z):
    p = {k[len("param_"):]: float(z[k]) for k in z.files if k.startswith("param_")}
    for k in ("min_mask_segments", "min_part_segments", "max_instance_num"):
        p[k] = int(p[k])
    return p


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    dbg = {}
    out = SR.freemask_segments_ref(z["key_feats"], z["key_coords"], z["key_segment_ids"], z["seg_connectivity"],
                                   z["scene_extent"], debug=dbg, **golden_params(z))
    return z, out, dbg


def test_restatement_reproduces_the_reference_run(golden):
    z, (soft, maskness, query, root), dbg = golden
    assert 65 <= len(dbg["unique_segments"]) <= 200
    assert query.tolist() == z["query_segment"].tolist()        # the reference's survivors in the reference's order
    assert root.tolist() == z["part_root"].tolist()
    print("maskness err", np.abs(maskness - z["maskness"]).max(), "soft err", np.abs(soft - z["soft_masks"]).max())
    assert np.abs(maskness - z["maskness"]).max() <= 1e-5
    assert soft.shape == z["soft_masks"].shape
    assert np.abs(soft - z["soft_masks"]).max() <= 1e-5
    # what the scene was planted for
    assert (dbg["idx"] == -1).any()                             # a dropped segment's voxels
    assert not dbg["extent_ok"].all() and dbg["extent_ok"].any()  # the room's rows fail the extent filter
    pairs = {}
    for q, r in zip(query, root):
        pairs.setdefault(int(q), []).append(int(r))
    assert any(len(v) == 2 for v in pairs.values())            # one query, two surviving parts
    assert len(set(root.tolist())) < len(root)                  # two survivors on one part: kept by voxel IoU only


def test_pooled_input_ids_are_the_key_ids(golden):
    z = golden[0]
    coords, ids = SR.maxpool_ids(z["in_coords"], z["in_segment_ids"], 1)
    order = np.lexsort(z["key_coords"].T[::-1])
    assert np.array_equal(coords, z["key_coords"][order]) and np.array_equal(ids, z["key_segment_ids"][order])


def check_segment_level(seg_masks, idx, coords):
    S = seg_masks.shape[1]
    w, lo, hi = SR.segment_tables(idx, coords, S)
    vmasks = SR.remap(seg_masks.astype(np.float64), idx) > 0
    count, box_lo, box_hi, inter = SR.segment_level_quantities(seg_masks, w, lo, hi)
    vlo, vhi = FR.mask_extent(vmasks, coords)
    assert np.array_equal(count, vmasks.sum(1))
    assert np.array_equal(box_lo, vlo) and np.array_equal(box_hi, vhi)
    assert np.array_equal(inter, vmasks.astype(np.int64) @ vmasks.astype(np.int64).T)


def test_voxel_level_equals_segment_level(golden):
    z, _, dbg = golden
    idx, coords = dbg["idx"], z["key_coords"].astype(np.int64)
    check_segment_level(dbg["seg_masks"], idx, coords)          # every row of the golden scene after the split
    assert np.array_equal(dbg["voxel_masks"], SR.remap(dbg["seg_masks"].astype(np.float64), idx) > 0)
    rng = np.random.default_rng(5)
    S = len(dbg["unique_segments"])
    rand = rng.random((40, S)) < rng.uniform(0.02, 0.9, (40, 1))
    rand[0], rand[1] = False, True                               # the empty and the full union
    check_segment_level(rand, idx, coords)
    # segment-count IoU and voxel-count IoU do differ on this scene
    w = SR.segment_tables(idx, coords, S)[0]
    assert len(set(w.tolist())) > 2


def test_select_picks_the_restatements_survivors(golden):
    z, _, dbg = golden
    p = golden_params(z)
    a, uniq = dbg["a"], dbg["unique_segments"]
    masks = a >= p["hard_mask_threshold"]
    cand = np.nonzero(masks.sum(1) > p["min_mask_segments"])[0]
    rows, query, root = SR.split_rows(a, masks, cand, dbg["adj"], p["min_part_segments"])    # candidate order
    seg_masks = rows >= p["hard_mask_threshold"]
    vmasks = SR.remap(rows, dbg["idx"]) >= p["hard_mask_threshold"]
    pairs = list(zip(uniq[query].tolist(), uniq[root].tolist()))
    assert len(set(pairs)) == len(pairs)

    def want_for(ext, q):
        _, _, qs, rs = SR.freemask_segments_ref(z["key_feats"], z["key_coords"], z["key_segment_ids"],
                                                z["seg_connectivity"], ext, **q)
        return np.array([pairs.index(pr) for pr in zip(qs.tolist(), rs.tolist())], np.int64)

    TH.check_select((rows * seg_masks).sum(1), seg_masks.sum(1), vmasks, z["key_coords"], z["scene_extent"], p, want_for)


def test_triple_bridge_graph_documents_deviation_d(golden):
    z = golden[0]
    ids, conn, ref_label = z["bridge_ids"], z["bridge_conn"], z["bridge_reference_label"]
    adj = SR.undirected_adjacency(conn, ids)
    label = SR.components(np.ones(len(ids), bool), adj)
    assert ids[label].tolist() == [1, 1, 1, 4, 1]               # 5 joins 1, 2 and 3; 4 stands alone
    assert ids[label].tolist() != ref_label.tolist()            # the reference leaves {3} apart
    assert ref_label.tolist() == [1, 1, 3, 4, 1]
    # one-directional pairs, self pairs and unknown ids
    adj = SR.undirected_adjacency(np.array([[2, 1], [3, 3], [3, 99], [99, 4]]), ids)
    assert [sorted(a) for a in adj] == [[1], [0], [], [], []]
