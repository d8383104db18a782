"""Axis-aligned 3D box AP of the validation loop (reference utils/votenet_utils/eval_det.py `eval_det` with
`use_07_metric=False` and metric_util.calc_iou; boxes built at trainer/trainer.py:668-697).

Boxes are (centre xyz, extent xyz).  Detections of one class are ranked by descending score over all scenes; each takes
the GT box of its scene with the highest IoU (the first of equal ones) and is a true positive when that IoU exceeds the
threshold and the GT box is not taken yet.  AP is the area under the monotone precision envelope (VOC 2010+)."""
from __future__ import annotations

import numpy as np
import torch


def box_iou(box, gts):
    """IoU of one box f64[6] with every box of gts f64[G, 6]; 0 where the boxes do not overlap on all three axes."""
    hi = np.minimum(box[0:3] + box[3:6] / 2, gts[:, 0:3] + gts[:, 3:6] / 2)
    lo = np.maximum(box[0:3] - box[3:6] / 2, gts[:, 0:3] - gts[:, 3:6] / 2)
    overlap = (hi > lo).all(1)
    inter = (hi - lo).prod(1)
    union = box[3:6].prod() + gts[:, 3:6].prod(1) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(overlap, 1.0 * inter / union, 0.0)


def voc_ap(rec, prec):
    """Area under the precision envelope, summed where recall changes."""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def eval_det_cls(pred, gt, ovthresh=0.25):
    """One class.  pred {scene: [(box, score)]}, gt {scene: [box]} -> (rec, prec, ap)."""
    gt_boxes, taken, npos = {}, {}, 0
    for sid, boxes in gt.items():
        gt_boxes[sid] = np.array(boxes).astype(float)
        taken[sid] = [False] * len(boxes)
        npos += len(boxes)
    scene_of, conf, bb = [], [], []
    for sid, dets in pred.items():
        for box, score in dets:
            scene_of.append(sid)
            conf.append(score)
            bb.append(box)
    conf = np.array(conf)
    order = np.argsort(-conf)
    bb = np.array(bb)[order, ...]
    nd = len(scene_of)
    tp, fp = np.zeros(nd), np.zeros(nd)
    for d in range(nd):
        sid = scene_of[order[d]]
        gts = gt_boxes.get(sid)
        if gts is None or gts.size == 0:
            fp[d] = 1.0
            continue
        iou = box_iou(bb[d, ...].astype(float), gts)
        j = int(np.argmax(iou))                     # first of the maxima (the reference's strict `>` scan)
        if iou[j] > ovthresh and not taken[sid][j]:
            tp[d] = 1.0
            taken[sid][j] = True
        else:
            fp[d] = 1.0
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    rec = tp / (float(npos) + 1e-5)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec)


def eval_det(pred_all, gt_all, ovthresh=0.25):
    """pred_all {scene: [(class, box, score)]}, gt_all {scene: [(class, box)]} -> (rec, prec, ap) dicts by class, in
    the order classes first appear (predictions first, then GT)."""
    pred, gt = {}, {}
    for sid, dets in pred_all.items():
        for cls, box, score in dets:
            pred.setdefault(cls, {}).setdefault(sid, []).append((box, score))
            gt.setdefault(cls, {}).setdefault(sid, [])
    for sid, boxes in gt_all.items():
        for cls, box in boxes:
            gt.setdefault(cls, {}).setdefault(sid, []).append(box)
            pred.setdefault(cls, {}).setdefault(sid, [])
    rec, prec, ap = {}, {}, {}
    for cls in gt:
        rec[cls], prec[cls], ap[cls] = eval_det_cls(pred[cls], gt[cls], ovthresh)
    return rec, prec, ap


def pred_box_list(pred_boxes):
    """eval_step's pred_boxes f64[K', 8] (class, centre, extent, score) -> [(class, box f64[6], score f32)]: the
    scores are the f32 pred_scores (exact in f64), ranked as the reference ranks its f32 scores."""
    return [(int(r[0]), np.asarray(r[1:7], np.float64), np.float32(r[7])) for r in np.asarray(pred_boxes)]


def gt_boxes(target_full_b, full_res_coords_b, label_offset=0):
    """GT boxes of one scene on the device (postprocess.mask_boxes): target_full_b {"labels" [T], "masks" bool [T, N]},
    full_res_coords_b [N, 3] -> [(class, box f64[6])] of the non-empty instances whose label is not 255."""
    from ..trainer.postprocess import mask_boxes
    masks = target_full_b["masks"]
    labels = np.asarray(torch.as_tensor(target_full_b["labels"]).cpu()).astype(np.int64) + label_offset
    keep = np.nonzero(labels != 255)[0]
    if keep.size == 0:
        return []
    dev = masks.device
    m = masks.index_select(0, torch.as_tensor(keep, device=dev)).T.bool()
    rows = mask_boxes(m, torch.as_tensor(np.asarray(full_res_coords_b), device=dev), labels[keep],
                      np.zeros(keep.size))
    return [(int(r[0]), np.asarray(r[1:7], np.float64)) for r in rows]
