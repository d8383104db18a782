"""CPU: the validation metrics' host half (unscene3d_amd/evaluation) against the reference evaluators' own outputs on
synthetic scenes (tests/golden/instance_ap.npz, tests/golden/make_golden_eval.py): ScanNet instance AP / AR
(benchmark/evaluate_semantic_instance.py), its result CSV, VoteNet box AP (utils/votenet_utils/eval_det.py) and the
val_* dict of trainer.eval_instance_epoch_end.

The count tables the device computes (ops.mask_gt_overlap) are restated here in numpy; everything downstream of them
is the product code.  Every comparison is exact: the matching and the curves repeat the reference's float64 operations
on the same integers, in the same order."""
import os

import numpy as np
import pytest

from unscene3d_amd.evaluation import (ClassSet, InstanceAPEvaluator, SceneGT, eval_det, load_gt_ids,
                                      validation_results)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_ap.npz")
RUNS = ("multi", "freemask")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def overlap_counts(masks, slot, nslots):
    """numpy statement of ops.mask_gt_overlap: int64 [K+1, nslots]."""
    n, k = masks.shape
    out = np.zeros((k + 1, nslots), np.int64)
    for j in range(k):
        out[j] = np.bincount(slot[masks[:, j] != 0], minlength=nslots)
    out[k] = np.bincount(slot, minlength=nslots)
    return out


def class_set(g, run):
    p = f"{run}__"
    names = dict(zip(g[p + "label_ids"].tolist(), g[p + "label_names"].tolist()))
    return ClassSet(g[p + "class_names"].tolist(), g[p + "class_ids"].tolist(), label_names=names)


def scenes(g, run):
    for i, name in enumerate(g[f"{run}__scenes"].tolist()):
        q = f"{run}__{i}__"
        n, k = int(g[q + "n"]), int(g[q + "k"])
        masks = np.unpackbits(g[q + "masks_packed"], axis=0, count=n).astype(bool)[:, :k]
        yield name, q, g[q + "gt_ids"].astype(np.int64), masks


def host_evaluator(g, run):
    ev = InstanceAPEvaluator(class_set(g, run))
    bbox_preds, bbox_gt = {}, {}
    for name, q, gt_ids, masks in scenes(g, run):
        sg = SceneGT(gt_ids, ev.class_set)
        counts = overlap_counts(masks, sg.slot, sg.nslots) if masks.shape[1] else None
        ev.add_scene_counts(name, counts, g[q + "scores"], g[q + "classes"], gt_ids=gt_ids)
        bbox_preds[name] = [(int(r[0]), r[1:7], np.float32(r[7])) for r in g[q + "pred_boxes"]]
        bbox_gt[name] = [(int(r[0]), r[1:7]) for r in g[q + "gt_boxes"]]
    return ev, bbox_preds, bbox_gt


def assert_same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True), np.nanmax(np.abs(a - b))


@pytest.mark.parametrize("run", RUNS)
def test_ap_ar_and_csv_equal_reference(gold, run):
    ev, _, _ = host_evaluator(gold, run)
    r = ev.compute()
    assert r["ap"].shape == (1, len(ev.class_set.ids), 10)
    assert_same(r["ap"], gold[f"{run}__ap"])
    assert_same(r["ar"], gold[f"{run}__ar"])
    assert [",".join(row) for row in ev.result_rows()] == gold[f"{run}__csv"].tolist()


@pytest.mark.parametrize("run", RUNS)
def test_box_ap_equals_reference(gold, run):
    _, bp, bg = host_evaluator(gold, run)
    for th in ("50", "25"):
        rec, prec, ap = eval_det(bp, bg, ovthresh=float(th) / 100)
        p = f"{run}__box{th}_"
        assert list(ap) == gold[p + "classes"].tolist()
        assert_same([ap[c] for c in ap], gold[p + "ap"])
        assert [len(rec[c]) for c in ap] == gold[p + "len"].tolist()
        assert_same(np.concatenate([rec[c] for c in ap]), gold[p + "rec"])
        assert_same(np.concatenate([prec[c] for c in ap]), gold[p + "prec"])


@pytest.mark.parametrize("run", RUNS)
def test_val_dict_equals_reference(gold, run):
    ev, bp, bg = host_evaluator(gold, run)
    d = validation_results(ev, bp, bg)
    want = dict(zip(gold[f"{run}__val_keys"].tolist(), gold[f"{run}__val_values"].tolist()))
    assert sorted(d) == sorted(want)
    for k in want:
        assert d[k] == want[k], (k, d[k], want[k])
    assert "val_mean_ap_50" in d and "val_mean_box_ap_50" in d


def test_fixture_covers_the_cases(gold):
    """The golden scenes exercise the branches the issue lists (guards against a fixture regenerated too small)."""
    free = list(scenes(gold, "freemask"))
    assert any(m.shape[1] == 0 for _, _, _, m in free)                          # a scene without predictions
    assert any((ids // 1000 != 1).all() for _, _, ids, _ in free)               # a scene without GT
    cls = np.concatenate([gold[q + "classes"] for _, q, _, _ in free])
    assert {0, 1} <= set(cls.tolist())
    sizes = np.concatenate([m.sum(0) for _, _, _, m in free])
    assert (sizes < 100).any() and (sizes >= 100).any()
    scores = np.concatenate([gold[q + "scores"] for _, q, _, _ in free])
    assert np.unique(scores).size < scores.size                                 # tied scores
    gsz = np.concatenate([np.unique(ids[ids // 1000 == 1], return_counts=True)[1] for _, _, ids, _ in free])
    assert (gsz < 100).any()
    assert len(gold["multi__class_ids"]) == 18


def test_empty_box_evaluation_returns_empty_dict():
    ev = InstanceAPEvaluator(ClassSet(["foreground"], [1]))
    assert validation_results(ev, {}, {}) == {}


def test_load_gt_ids_round_trip(tmp_path):
    ids = np.array([0, 1001, 1001, 2003, 0, 39017, -1], np.int64)
    p = tmp_path / "scene0000_00.txt"
    p.write_text("\n".join(str(int(v)) for v in ids) + "\n")
    got = load_gt_ids(str(p))
    assert got.dtype == np.int64 and np.array_equal(got, ids)


def test_scene_gt_slots():
    cs = ClassSet(["a", "b"], [1, 3])
    ids = np.array([3002, 0, 1001, 2005, 1001, 3002, 1000, 7], np.int64)
    sg = SceneGT(ids, cs)
    assert sg.inst_ids.tolist() == [1000, 1001, 3002]
    assert sg.nslots == 5 and sg.void_slot == 4
    assert sg.slot.tolist() == [2, 4, 1, 4, 1, 2, 0, 4]
