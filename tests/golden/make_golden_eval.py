#!/usr/bin/env python
"""Golden vectors of the validation metrics — runs ONLY where the reference tree exists (the build container).

Imports the reference's ScanNet instance evaluator (benchmark/evaluate_semantic_instance.py, with `plyfile` and
`imageio` stubbed: neither is installed and neither is used on this path) and its VoteNet box evaluator
(utils/votenet_utils/eval_det.py, `trimesh` stubbed), runs them on small synthetic scenes and stores inputs and outputs
as data in tests/golden/instance_ap.npz.  Nothing from the reference is copied.

    python tests/golden/make_golden_eval.py

Two runs: "multi" uses the evaluator module's own 18-class table (its names and ids are stored as data) and runs first,
because evaluate(dataset="freemask") rewrites the module's class globals; "freemask" is the self-training setting.
The scenes cover tied scores, several predictions on one GT, predictions and GT instances below 100 points,
void-heavy predictions, a scene without GT, a scene without predictions and class-0 / class-1 predictions."""
import os
import statistics
import math
import sys
import tempfile
import types
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UNSCENE3D_REFERENCE", "/root/reference")


class _Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return MagicMock()


def import_reference():
    for name in ("plyfile", "imageio", "trimesh"):
        sys.modules.setdefault(name, _Stub(name))
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "utils", "votenet_utils"))     # eval_det imports box_util top-level
    import benchmark.evaluate_semantic_instance as esi
    from utils.votenet_utils.eval_det import eval_det
    return esi, eval_det


# ------------------------------------------------------------------ synthetic scenes
def make_scene(rng, n, labels, n_inst, no_gt=False, n_pred=30, pred_classes=(1,), class0_frac=0.0):
    """-> gt_ids i64[n], masks bool[n, K], scores f32[K], classes i64[K], coords f32[n, 3]."""
    coords = rng.uniform(0, 4, (n, 3)).astype(np.float32)
    gt = np.zeros(n, np.int64)
    perm = rng.permutation(n)                       # instances are scattered over the point order
    pos, insts, inst_lab = 0, [], []
    if not no_gt:
        for i in range(n_inst):
            size = int(rng.integers(30, 95)) if i % 5 == 4 else int(rng.integers(150, 1500))   # every 5th is small
            lab = int(labels[i % len(labels)])
            iid = lab * 1000 + i + 1
            idx = perm[pos:pos + size]
            pos += size
            gt[idx] = iid
            insts.append(idx)
            inst_lab.append(lab)
        # a few points of an id whose label is outside the evaluated classes: void
        gt[perm[pos:pos + 300]] = 99 * 1000 + 1
        pos += 300
    void_pts = np.nonzero((gt == 0) | (gt // 1000 == 99))[0]
    masks, pcls = [], []
    for j in range(n_pred):
        kind = j % 6
        m = np.zeros(n, bool)
        pcls.append(int(pred_classes[rng.integers(0, len(pred_classes))]))
        if insts and kind in (0, 1, 2):             # noisy copy of a GT instance; kind 1/2 reuse the same GT (duplicates)
            gi = (j // 6) % len(insts) if kind else (j // 3) % len(insts)
            src = insts[gi]
            if rng.random() < 0.85:
                pcls[-1] = inst_lab[gi]
            keep = src[rng.random(src.size) > rng.uniform(0.0, 0.5)]
            m[keep] = True
            m[rng.choice(n, int(rng.integers(0, src.size // 2 + 1)), replace=False)] = True
        elif kind == 3:                             # void-heavy
            m[rng.choice(void_pts, min(void_pts.size, int(rng.integers(100, 600))), replace=False)] = True
            if insts:
                src = insts[j % len(insts)]
                m[src[: max(1, src.size // 8)]] = True
        elif kind == 4:                             # below 100 points
            m[rng.choice(n, int(rng.integers(20, 99)), replace=False)] = True
        else:                                       # random, or covering a small GT instance
            if insts and j % 12 == 5:
                small = [s for s in insts if s.size < 100]
                src = small[0] if small else insts[0]
                m[src] = True
                m[rng.choice(void_pts, min(void_pts.size, 150), replace=False)] = True
            else:
                m[rng.choice(n, int(rng.integers(100, 2000)), replace=False)] = True
        masks.append(m)
    masks = np.stack(masks, 1) if masks else np.zeros((n, 0), bool)
    scores = np.round(rng.uniform(0.05, 1.0, n_pred), 1).astype(np.float32)      # one decimal: many ties
    classes = np.array(pcls, np.int64)
    classes[rng.random(n_pred) < class0_frac] = 0
    return gt, masks, scores, classes, coords


def boxes_of(mask_cols, coords):
    """(centre, extent) f64[6] of every non-empty column (as the reference's trainer builds them), and which."""
    out, ok = [], []
    for j in range(mask_cols.shape[1]):
        pts = coords[mask_cols[:, j]].astype(np.float64)
        ok.append(pts.shape[0] > 0)
        if pts.shape[0]:
            out.append(np.concatenate((pts.mean(0), pts.max(0) - pts.min(0))))
    return np.array(out).reshape(-1, 6), np.array(ok, bool)


def val_dict(box50, box25, csv_path, label_names, prefix="val"):
    """The dict eval_instance_epoch_end logs, assembled from the reference evaluators' outputs."""
    if len(box50[0]) == 0:
        return {}
    d = {f"{prefix}_mean_box_ap_25": sum(box25[2].values()) / len(box25[2]),
         f"{prefix}_mean_box_ap_50": sum(box50[2].values()) / len(box50[2])}
    for cid, v in box50[2].items():
        d[f"{prefix}_{label_names[cid]}_val_box_ap_50"] = v
    for cid, v in box25[2].items():
        d[f"{prefix}_{label_names[cid]}_val_box_ap_25"] = v
    with open(csv_path) as f:
        for row in f.read().splitlines()[1:]:
            name, _, ap, ap50, ap25 = row.split(",")[:5]
            d[f"{prefix}_{name}_val_ap"] = float(ap)
            d[f"{prefix}_{name}_val_ap_50"] = float(ap50)
            d[f"{prefix}_{name}_val_ap_25"] = float(ap25)
    for suffix, key in (("val_ap", "mean_ap"), ("val_ap_50", "mean_ap_50"), ("val_ap_25", "mean_ap_25")):
        d[f"{prefix}_{key}"] = statistics.mean([v for k, v in d.items() if k.endswith(suffix)])
    return {k: 0.0 if math.isnan(v) else float(v) for k, v in d.items()}


def run(esi, eval_det, tag, scenes, dataset, label_names, tmp, out):
    gt_dir = os.path.join(tmp, tag, "gt")
    os.makedirs(gt_dir)
    preds, bbox_preds, bbox_gt = {}, {}, {}
    for name, (gt, masks, scores, classes, coords) in scenes.items():
        with open(os.path.join(gt_dir, name + ".txt"), "w") as f:
            f.write("\n".join(str(int(v)) for v in gt) + "\n")
        preds[name] = {"pred_masks": masks, "pred_scores": scores, "pred_classes": classes}
        pb, pok = boxes_of(masks, coords)
        bbox_preds[name] = [(int(c), b, s) for c, b, s in zip(classes[pok], pb, scores[pok])]
        ids = [i for i in np.unique(gt) if i != 0]
        gcols = np.stack([gt == i for i in ids], 1) if ids else np.zeros((gt.size, 0), bool)
        gb, gok = boxes_of(gcols, coords)
        glab = np.array([i // 1000 for i in ids], np.int64)[gok]
        bbox_gt[name] = [(int(c), b) for c, b in zip(glab, gb) if c != 99]
    captured = {}
    real = esi.evaluate_matches

    def capture(matches):           # the first call is the whole split; per-scene calls (scene_metrics.csv) follow
        ap, ar = real(matches)
        captured.setdefault("ap", ap)
        captured.setdefault("ar", ar)
        return ap, ar

    esi.evaluate_matches = capture
    csv_path = os.path.join(tmp, tag, "result.txt")
    try:
        esi.evaluate(preds, gt_dir, csv_path, dataset=dataset)
    finally:
        esi.evaluate_matches = real
    box50 = eval_det(bbox_preds, bbox_gt, ovthresh=0.5, use_07_metric=False)
    box25 = eval_det(bbox_preds, bbox_gt, ovthresh=0.25, use_07_metric=False)
    p = f"{tag}__"
    out[p + "class_names"] = np.array(list(esi.CLASS_LABELS))
    out[p + "class_ids"] = np.array(esi.VALID_CLASS_IDS, np.int64)
    out[p + "label_ids"] = np.array(list(label_names), np.int64)
    out[p + "label_names"] = np.array(list(label_names.values()))
    out[p + "scenes"] = np.array(list(scenes))
    out[p + "ap"], out[p + "ar"] = captured["ap"], captured["ar"]
    with open(csv_path) as f:
        out[p + "csv"] = np.array(f.read().splitlines())
    for i, (name, (gt, masks, scores, classes, coords)) in enumerate(scenes.items()):
        q = f"{p}{i}__"
        out[q + "gt_ids"] = gt.astype(np.int32)
        out[q + "n"] = np.int64(masks.shape[0])
        out[q + "k"] = np.int64(masks.shape[1])
        out[q + "masks_packed"] = np.packbits(masks, axis=0)
        out[q + "scores"], out[q + "classes"] = scores, classes
        out[q + "pred_boxes"] = np.array([[c, *b, s] for c, b, s in bbox_preds[name]], np.float64).reshape(-1, 8)
        out[q + "gt_boxes"] = np.array([[c, *b] for c, b in bbox_gt[name]], np.float64).reshape(-1, 7)
    for th, res in (("50", box50), ("25", box25)):
        rec, prec, ap = res
        out[f"{p}box{th}_classes"] = np.array(list(ap), np.int64)
        out[f"{p}box{th}_ap"] = np.array([ap[c] for c in ap], np.float64)
        out[f"{p}box{th}_len"] = np.array([len(rec[c]) for c in ap], np.int64)
        out[f"{p}box{th}_rec"] = np.concatenate([rec[c] for c in ap]) if ap else np.zeros(0)
        out[f"{p}box{th}_prec"] = np.concatenate([prec[c] for c in ap]) if ap else np.zeros(0)
    vd = val_dict(box50, box25, csv_path, label_names)
    out[p + "val_keys"] = np.array(list(vd))
    out[p + "val_values"] = np.array(list(vd.values()), np.float64)
    print(tag, "mean ap / ap50 / ap25:", [vd.get(f"val_mean_ap{s}") for s in ("", "_50", "_25")],
          "box ap50:", vd.get("val_mean_box_ap_50"))


def main():
    esi, eval_det = import_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        # 18 classes: the evaluator module's own table, before evaluate(dataset="freemask") rewrites it
        ids18 = [int(i) for i in esi.VALID_CLASS_IDS]
        rng = np.random.default_rng(7)
        multi = {}
        for s in range(2):
            multi[f"scene09{s:02d}_00"] = make_scene(rng, 12000 + 4000 * s, ids18[s::2][:9], 12, n_pred=36,
                                                     pred_classes=ids18, class0_frac=0.05)
        names18 = dict(zip(ids18, esi.CLASS_LABELS))
        names18[0] = "background"
        run(esi, eval_det, "multi", multi, "scannet", names18, tmp, out)

        rng = np.random.default_rng(11)
        free = {}
        free["scene0001_00"] = make_scene(rng, 8000, [1], 10, n_pred=30, class0_frac=0.2)
        free["scene0002_00"] = make_scene(rng, 14000, [1], 16, n_pred=42, class0_frac=0.15)
        free["scene0003_00"] = make_scene(rng, 20000, [1], 24, n_pred=36, class0_frac=0.1)
        free["scene0004_00"] = make_scene(rng, 9000, [1], 0, no_gt=True, n_pred=12, class0_frac=0.1)   # no GT
        free["scene0005_00"] = make_scene(rng, 10000, [1], 8, n_pred=0)                                 # no predictions
        free["scene0006_00"] = make_scene(rng, 12000, [1], 12, n_pred=24, class0_frac=0.25)
        run(esi, eval_det, "freemask", free, "freemask", {0: "background", 1: "foreground"}, tmp, out)
    path = os.path.join(HERE, "instance_ap.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
