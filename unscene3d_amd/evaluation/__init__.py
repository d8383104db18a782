"""Validation metrics of the self-training loop: ScanNet instance mask AP / AR (instance_ap) and VoteNet axis-aligned
box AP (box_ap).  The [points]-sized part is one device histogram per scene (ops.mask_gt_overlap); the matching runs on
the host from the count tables."""
import math
import statistics

from .box_ap import eval_det, gt_boxes, pred_box_list
from .instance_ap import FREEMASK, OVERLAPS, ClassSet, InstanceAPEvaluator, SceneGT, load_gt_ids

__all__ = ["ClassSet", "FREEMASK", "OVERLAPS", "InstanceAPEvaluator", "SceneGT", "load_gt_ids", "eval_det",
           "gt_boxes", "pred_box_list", "validation_results"]


def validation_results(evaluator: InstanceAPEvaluator, bbox_preds, bbox_gt, prefix="val"):
    """The dict the reference's eval_instance_epoch_end logs (trainer/trainer.py:785-931, ScanNet / freemask branch):
    mean and per-class box AP at 0.25 / 0.5, per-class mask AP / AP50 / AP25 read back from the result rows'
    strings (float(str(x)): the identity on float64, NaN included), their means over classes (statistics.mean), and
    every NaN replaced by 0.  Empty when the box evaluation has no class (the reference returns early there)."""
    box50 = eval_det(bbox_preds, bbox_gt, ovthresh=0.5)
    box25 = eval_det(bbox_preds, bbox_gt, ovthresh=0.25)
    if len(box50[0]) == 0:
        return {}
    cs = evaluator.class_set
    out = {f"{prefix}_mean_box_ap_25": sum(v for v in box25[2].values()) / len(box25[2]),
           f"{prefix}_mean_box_ap_50": sum(v for v in box50[2].values()) / len(box50[2])}
    for cid, v in box50[2].items():
        out[f"{prefix}_{cs.label_name(cid)}_val_box_ap_50"] = v
    for cid, v in box25[2].items():
        out[f"{prefix}_{cs.label_name(cid)}_val_box_ap_25"] = v
    for row in evaluator.result_rows()[1:]:
        name, ap, ap50, ap25 = row[0], row[2], row[3], row[4]
        out[f"{prefix}_{name}_val_ap"] = float(ap)
        out[f"{prefix}_{name}_val_ap_50"] = float(ap50)
        out[f"{prefix}_{name}_val_ap_25"] = float(ap25)
    for suffix in ("val_ap", "val_ap_50", "val_ap_25"):
        out[f"{prefix}_mean_{suffix[4:]}"] = statistics.mean([v for k, v in out.items() if k.endswith(suffix)])
    return {k: 0.0 if math.isnan(v) else v for k, v in out.items()}
