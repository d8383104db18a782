"""CPU: the float64 restatement tests/freemask_ref.py reproduces the reference's own run (tests/golden/freemask.npz,
written by tests/golden/make_golden_freemask.py from the reference's cosine_sim and matrix_nms), the inputs of the
GPU kernel tests meet the condition those tests put on them, and the package's selection tail (`_select`, torch
operators only) picks the restatement's survivors from the restatement's candidates."""
import os

import numpy as np
import pytest
import torch

import freemask_cases as FC
import freemask_ref as FR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freemask.npz")


def _params(z):
    p = {k[len("param_"):]: float(z[k]) for k in z.files if k.startswith("param_")}
    p["min_mask_points"], p["max_instance_num"] = int(p["min_mask_points"]), int(p["max_instance_num"])
    return p


def test_ref_reproduces_the_reference_run():
    z = np.load(GOLDEN)
    soft, maskness, qidx = FR.freemask_ref(z["key_feats"], z["key_coords"], z["query_feats"], z["scene_extent"],
                                           **_params(z))
    assert qidx.tolist() == z["query_index"].tolist()           # the reference's survivors, in its order
    assert np.abs(maskness - z["maskness"]).max() <= 1e-6
    assert soft.shape == z["soft_masks"].shape
    assert np.abs(soft - z["soft_masks"]).max() <= 1e-6
    # the whole-room cluster (5) made candidates, and none of them survived
    assert (z["query_cluster"] == 5).sum() == 64
    assert sorted(z["query_cluster"][qidx].tolist()) == [0, 1, 2, 3, 4]


def test_ref_extent_filter_is_what_drops_the_room():
    z = np.load(GOLDEN)
    p = _params(z)
    p["instance_to_scene_max_ratio"] = 2.0                      # filter off: the room's best mask survives as well
    _, _, qidx = FR.freemask_ref(z["key_feats"], z["key_coords"], z["query_feats"], z["scene_extent"], **p)
    assert sorted(z["query_cluster"][qidx].tolist()) == [0, 1, 2, 3, 4, 5]


# `_select` on what the restatement computes.  The three parameter sets: the golden ones, a cut at 3 masks, and a scene
# extent scaled down until no mask passes the extent filter ("none left -> all stay"); 2.0 is above every maskness.
SELECT_SETS = [dict(), dict(max_instance_num=3), dict(extent_scale=1e-3)]


def check_select(sums, counts, masks, coords, scene_extent, p, want_for):
    """sums f64[n], counts int[n], masks bool[n,K] of the candidates in candidate order, coords int[K,3];
    want_for(parameters) -> the restatement's survivors as positions in the candidate list."""
    from unscene3d_amd.pseudo_masks.freemask import _select
    m64 = sums / counts
    maskness = torch.from_numpy(sums).float() / torch.from_numpy(counts)        # f32 sum / integer, as on the device
    assert maskness.dtype == torch.float32
    # no tie that f32 and f64 order differently, in any subset of the candidates
    assert np.array_equal(np.argsort(-maskness.numpy(), kind="stable"), np.argsort(-m64, kind="stable"))
    lo, hi = (torch.from_numpy(b).int() for b in FR.mask_extent(masks, coords))
    vox = masks.sum(1)

    def nms(order):
        o = order.numpy()
        return torch.from_numpy(FR.greedy_nms(masks[o], vox[o], p["nms_thr"]))

    def run(extent_scale=1.0, **over):
        q = {**p, **over}
        ext = np.asarray(scene_extent, np.float64) * extent_scale
        got = _select(maskness, torch.arange(len(sums)), lo, hi, torch.from_numpy(ext), nms,
                      instance_to_scene_max_ratio=q["instance_to_scene_max_ratio"],
                      max_instance_num=q["max_instance_num"], nms_maskness_threshold=q["nms_maskness_threshold"])
        return got, want_for(ext, q), ((hi - lo)[:, :2].double() / torch.from_numpy(ext)[:2] > q[
            "instance_to_scene_max_ratio"]).any(1)

    for i, over in enumerate(SELECT_SETS):
        (got_m, got_rows), want, too_big = run(**over)
        assert too_big.any() and (bool(too_big.all()) == (i == 2))              # set 2 is the "all stay" branch
        assert got_rows.dtype == torch.int64 and got_rows.tolist() == want.tolist() and len(want) >= 3
        assert len(want) == 3 or i != 1
        assert np.abs(got_m.numpy() - m64[want]).max() <= 1e-6                   # two f32 roundings of a value <= 1
    got, want, _ = run(nms_maskness_threshold=2.0)
    assert got is None and len(want) == 0


def test_select_picks_the_restatements_survivors():
    z = np.load(GOLDEN)
    p = _params(z)
    a, _, _, _ = FR.cosine_rows(z["key_feats"], z["query_feats"])
    masks = a >= p["hard_mask_threshold"]
    cand = np.nonzero(masks.sum(1) > p["min_mask_points"])[0]

    def want_for(ext, q):
        qidx = FR.freemask_ref(z["key_feats"], z["key_coords"], z["query_feats"], ext, **q)[2]
        return np.searchsorted(cand, qidx)

    check_select((a[cand] * masks[cand]).sum(1), masks[cand].sum(1), masks[cand], z["key_coords"], z["scene_extent"], p,
                 want_for)


def test_ref_nms_rules():
    # IoU exactly 1/2 is kept; 2 inter = union + 1 is suppressed; a dead mask suppresses nothing; empty later mask dies
    def rows(K, *spans):
        m = np.zeros((len(spans), K), bool)
        for i, (a, b) in enumerate(spans):
            m[i, a:b] = True
        return m
    m = rows(12, (0, 6), (3, 9))                                # inter 3, union 9
    assert FR.greedy_nms(m, m.sum(1)).tolist() == [True, True]
    m = rows(12, (0, 4), (2, 6))                                # inter 2, union 6: 1/3
    assert FR.greedy_nms(m, m.sum(1)).tolist() == [True, True]
    m = rows(12, (0, 4), (0, 2))                                # inter 2, union 4: exactly 1/2 -> kept
    assert FR.greedy_nms(m, m.sum(1)).tolist() == [True, True]
    m = rows(12, (0, 5), (0, 3))                                # inter 3, union 5: 2 * 3 = 5 + 1 -> suppressed
    assert FR.greedy_nms(m, m.sum(1)).tolist() == [True, False]
    m = rows(20, (0, 10), (3, 12), (6, 14))                     # A,B 7/12: B dies; B,C 6/11 would kill C; A,C 4/14: C lives
    assert FR.greedy_nms(m, m.sum(1)).tolist() == [True, False, True]
    m = rows(8, (0, 4), (0, 0))                                 # union > 0: 0/4 -> the empty mask is kept by that rule
    assert FR.greedy_nms(m, m.sum(1)).tolist() == [True, True]
    m = rows(8, (0, 0), (0, 0))                                 # union == 0 -> killed by the else-branch
    assert FR.greedy_nms(m, m.sum(1)).tolist() == [True, False]


@pytest.mark.parametrize("shape", FC.SHAPES + FC.EXTRA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_case_inputs_meet_the_skip_condition(shape):
    Q, K, C = shape
    fk, fq, _ = FC.make_case(Q, K, C)
    assert np.all(fk == 0, 1).any()
    a, lo, hi, _ = FR.cosine_rows(fk, fq)
    share = FC.skip_mask(a, lo, hi, fq, C).mean()
    print(f"{shape}: share of entries within delta_row of the threshold: {share:.3g}")
    assert share <= FC.SKIP_SHARE_MAX
    if shape in FC.ZERO_QUERY:
        q = FC.ZERO_QUERY[shape]
        assert not fq[q].any() and not (a[q] >= FC.THRESHOLD).any()
