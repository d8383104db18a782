"""ScanNet instance-segmentation AP (reference benchmark/evaluate_semantic_instance.py: `evaluate` with a `gt_dict`,
`assign_instances_for_scan_with_gt`, `evaluate_matches`, `compute_metric_averages`, `write_result_file`).

The reference intersects every predicted mask with every GT instance by an O(K·G·N) loop of numpy boolean ops.  Here
the only [points]-sized work is one device histogram per scene (`ops.mask_gt_overlap`): every point carries the slot
of its GT instance, and the table counts, for each mask column, its points in each slot.  Every quantity the matching
needs is a sum of table entries:

    pred vert_count        = row j summed over all slots
    void_intersection      = row j at the void slot
    intersection with GT g = row j at slot g
    GT vert_count          = row K (all points) at slot g

The greedy matching, the precision/recall curve and the averages then run on the host in float64 on these integers,
in the reference's order, so the numbers are the reference's."""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import numpy as np
import torch

# IoU thresholds: 0.5, 0.55, ..., 0.9, then 0.25 (the reference's opt['overlaps'], built the same way)
OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
_O50 = np.where(np.isclose(OVERLAPS, 0.5))
_O25 = np.where(np.isclose(OVERLAPS, 0.25))
_O_NOT25 = np.where(np.logical_not(np.isclose(OVERLAPS, 0.25)))


@dataclass(frozen=True)
class ClassSet:
    """The evaluated classes: `names[i]` has the GT label id `ids[i]` (instance id = label * 1000 + instance).
    `label_names` names every label the model can predict (box AP keys, which cover predicted labels outside the
    evaluated set too); it defaults to names/ids."""
    names: tuple
    ids: tuple
    label_names: dict = field(default=None)

    def __post_init__(self):
        object.__setattr__(self, "names", tuple(str(n) for n in self.names))
        object.__setattr__(self, "ids", tuple(int(i) for i in self.ids))
        if len(self.names) != len(self.ids) or len(set(self.ids)) != len(self.ids) or not self.ids:
            raise ValueError("ClassSet: names and ids must be non-empty, of equal length, ids unique")
        ln = dict(zip(self.ids, self.names))
        ln.update({int(k): str(v) for k, v in (self.label_names or {}).items()})
        object.__setattr__(self, "label_names", ln)

    def label_name(self, label_id) -> str:
        return self.label_names.get(int(label_id), str(int(label_id)))


# the self-training setting (`dataset="freemask"`): one evaluated class; the model also predicts label 0 (background)
FREEMASK = ClassSet(["foreground"], [1], label_names={0: "background", 1: "foreground"})


def load_gt_ids(path) -> np.ndarray:
    """`instance_gt/<split>/<scene>.txt`: one integer per line, label * 1000 + instance -> int64[N]."""
    with open(path) as f:
        return np.array(f.read().splitlines(), dtype=np.int64)


class SceneGT:
    """Host preparation of one scene's GT ids (once per scene): the GT instances (non-zero ids whose label is in the
    class set, ascending id) and the slot of every point: instance g -> g, a non-void point outside every instance ->
    G, void (label not in the class set) -> G + 1 (the last slot)."""

    def __init__(self, gt_ids, class_set: ClassSet):
        gt_ids = np.asarray(gt_ids, dtype=np.int64).reshape(-1)
        uniq, inv = np.unique(gt_ids, return_inverse=True)
        valid = np.isin(uniq // 1000, np.asarray(class_set.ids, dtype=np.int64))
        inst = valid & (uniq != 0)
        self.n = int(gt_ids.shape[0])
        self.inst_ids = uniq[inst]                                   # [G]
        self.inst_label = self.inst_ids // 1000
        g = int(self.inst_ids.shape[0])
        self.nslots = g + 2
        self.void_slot = g + 1
        slot_of_uniq = np.where(inst, np.cumsum(inst) - 1, np.where(valid, g, g + 1))
        self.slot = slot_of_uniq[inv.reshape(-1)].astype(np.int32)
        self.sizes = np.bincount(self.slot, minlength=self.nslots).astype(np.int64)   # used when a scene has no masks


def _scene_classes(table, gt: SceneGT, scores, classes, class_set: ClassSet, min_region_size: int):
    """Per class (class-set order) of one scene: the GT instances and the predictions that the reference keeps, with
    their intersections — the content of its gt2pred / pred2gt dicts, as arrays.  table: int64 [K+1, nslots] or None."""
    g = gt.nslots - 2
    if table is None:
        k, gt_vc = 0, gt.sizes[:g]
        vc = void = np.zeros(0, np.int64)
        inter = np.zeros((0, g), np.int64)
    else:
        k = table.shape[0] - 1
        gt_vc = table[k, :g]
        vc = table[:k].sum(1)
        void = table[:k, gt.void_slot]
        inter = table[:k, :g]
    classes = np.asarray(classes).reshape(-1).astype(np.int64)
    scores = np.asarray(scores).reshape(-1)
    if classes.shape[0] != k or scores.shape[0] != k:
        raise ValueError(f"pred_classes / pred_scores must have one entry per mask column ({k})")
    out = []
    for cid in class_set.ids:
        gsel = np.nonzero(gt.inst_label == cid)[0]
        psel = np.nonzero((classes == cid) & (vc >= min_region_size))[0]
        out.append({
            "gt_id": gt.inst_ids[gsel], "gt_vc": gt_vc[gsel],
            "conf": scores[psel].astype(np.float64), "vc": vc[psel], "void": void[psel],
            "inter": inter[np.ix_(psel, gsel)],
        })
    return out


def _pr_ap(y_true, y_score, hard_fn):
    """Average precision / recall of one class at one threshold from the scored true/false entries (the reference's
    curve: unique score thresholds, an artificial first point, step widths from a [-0.5, 0, 0.5] convolution)."""
    order = np.argsort(y_score)
    ys, cs = y_score[order], np.cumsum(y_true[order])
    _, first = np.unique(ys, return_index=True)
    total_true = cs[-1] if len(cs) > 0 else 0
    below = np.append(cs, 0)[first - 1]                   # true entries with a lower score (index -1 -> 0)
    tp = total_true - below
    fp = len(ys) - first - tp
    fn = below + hard_fn
    precision = np.append(tp / (tp + fp), 1.0)
    recall = np.append(tp / (tp + fn), 0.0)
    r = np.concatenate(([recall[0]], recall, [0.0]))
    widths = np.convolve(r, [-0.5, 0, 0.5], "valid")
    return np.dot(precision, widths), np.dot(recall, widths)


def _prepare(c, min_region_size):
    """Threshold-independent arrays of one scene and class: IoU of every (prediction, GT) pair with a common point,
    the GT instances that count, and each prediction's ignored share (void + group / small GT intersections)."""
    inter, gt_vc, vc = c["inter"], c["gt_vc"], c["vc"]
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter.astype(np.float64) / (gt_vc[None, :] + vc[:, None] - inter)           # [P, G]
    iou[inter <= 0] = -np.inf                                                               # no common point: no pair
    small = (c["gt_id"] < 1000).astype(np.int64) + (gt_vc < min_region_size).astype(np.int64)
    ignore = c["void"] + (inter * small[None, :]).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = ignore.astype(np.float64) / vc
    keep = np.nonzero((c["gt_id"] >= 1000) & (gt_vc >= min_region_size))[0]
    return iou, keep, share, c["conf"]


def match_and_score(scenes, n_classes: int, min_region_size: int = 100):
    """evaluate_matches on per-scene class data (`_scene_classes`, scenes in insertion order) -> ap, ar [1, C, O]."""
    ap = np.zeros((1, n_classes, len(OVERLAPS)), float)
    ar = np.zeros((1, n_classes, len(OVERLAPS)), float)
    prepared = [[_prepare(sc[li], min_region_size) for li in range(n_classes)] for sc in scenes]
    for oi, th in enumerate(OVERLAPS):
        for li in range(n_classes):
            trues, scores = [], []
            hard_fn, has_gt, has_pred = 0, False, False
            for sc in prepared:
                iou, keep, share, conf = sc[li]
                hit = iou > th                                                              # [P, G]
                has_gt |= len(keep) > 0
                has_pred |= len(conf) > 0
                # GT side: greedy in GT order, then prediction order; a prediction matches at most one GT
                visited = np.zeros(len(conf), bool)
                matched_s, extra_s = [], []
                for gi in keep:
                    best, found = -np.inf, False
                    for p in np.nonzero(hit[:, gi])[0]:
                        if visited[p]:
                            continue
                        if found:           # a second match: the lower score is a false positive
                            extra_s.append(min(best, conf[p]))
                            best = max(best, conf[p])
                        else:
                            found, best, visited[p] = True, conf[p], True
                    if found:
                        matched_s.append(best)
                    else:
                        hard_fn += 1
                # prediction side: a prediction without any GT above the threshold is a false positive unless the
                # ignored share of its points exceeds the threshold
                fp_s = conf[~hit.any(1) & (share <= th)].tolist()
                trues += [1.0] * len(matched_s) + [0.0] * (len(extra_s) + len(fp_s))
                scores += matched_s + extra_s + fp_s
            if has_gt and has_pred:
                ap[0, li, oi], ar[0, li, oi] = _pr_ap(np.array(trues, float), np.array(scores, float), hard_fn)
            elif has_gt:
                ap[0, li, oi], ar[0, li, oi] = 0.0, float("nan")
            else:
                ap[0, li, oi], ar[0, li, oi] = float("nan"), 0.0
    return ap, ar


def metric_averages(values, class_names, metric="ap"):
    """compute_metric_averages: all_<m>, all_<m>_50%, all_<m>_25% and per class <m>, <m>50%, <m>25%."""
    d = {f"all_{metric}": np.nanmean(values[0, :, _O_NOT25]),
         f"all_{metric}_50%": np.nanmean(values[0, :, _O50]),
         f"all_{metric}_25%": np.nanmean(values[0, :, _O25]),
         "classes": {}}
    for li, name in enumerate(class_names):
        d["classes"][name] = {metric: np.average(values[0, li, _O_NOT25]),
                              f"{metric}50%": np.average(values[0, li, _O50]),
                              f"{metric}25%": np.average(values[0, li, _O25])}
    return d


class InstanceAPEvaluator:
    """Accumulates validation scenes and computes mask AP / AR.

    add_scene() issues one device histogram per scene and keeps the table on the device; GT preparation runs once
    per scene name and is cached (host metadata + device slot map).  compute() reads every table back with one
    synchronisation.  Adding a scene name twice replaces its predictions, as in the reference's dict."""

    def __init__(self, class_set: ClassSet = FREEMASK, min_region_size: int = 100):
        self.class_set = class_set
        self.min_region_size = int(min_region_size)
        self._gt = {}          # scene name -> (SceneGT, device slot tensor or None)
        self.reset()

    def reset(self):
        self._scenes = {}      # scene name -> (table: device tensor / np array / None, scores, classes)
        self._result = None

    def has_gt(self, name) -> bool:
        return name in self._gt

    def _scene_gt(self, name, gt_ids, device=None):
        ent = self._gt.get(name)
        if ent is None:
            if gt_ids is None:
                raise KeyError(f"no GT ids for scene {name!r}")
            ent = [SceneGT(gt_ids, self.class_set), None]
            self._gt[name] = ent
        if device is not None and ent[1] is None:
            ent[1] = torch.from_numpy(ent[0].slot).to(device)
        return ent

    @staticmethod
    def _host(x):
        return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)

    def add_scene(self, name, instances, gt_ids=None):
        """instances: one dict as eval_step returns it (pred_masks bool [N_full, K] on the device, pred_scores,
        pred_classes).  gt_ids: int64 [N_full] (label * 1000 + instance); may be omitted once the scene is cached."""
        masks = instances["pred_masks"]
        gt, slot = self._scene_gt(name, gt_ids, device=masks.device)
        if masks.shape[0] != gt.n:
            raise ValueError(f"scene {name!r}: {masks.shape[0]} mask rows, {gt.n} GT ids")
        from .. import ops
        table = ops.mask_gt_overlap(masks, slot, gt.nslots) if masks.shape[1] > 0 else None
        self._scenes[name] = (table, self._host(instances["pred_scores"]), self._host(instances["pred_classes"]))
        self._result = None

    def add_scene_counts(self, name, counts, pred_scores, pred_classes, gt_ids=None):
        """Host entry: the scene's count table (int [K+1, nslots] as ops.mask_gt_overlap returns it for
        SceneGT(gt_ids).slot), its scores and classes."""
        self._scene_gt(name, gt_ids)
        self._scenes[name] = (None if counts is None or counts.shape[0] <= 1 else counts,
                              self._host(pred_scores), self._host(pred_classes))
        self._result = None

    def compute(self):
        """-> {"ap", "ar": float64 [1, C, O], "avg_ap", "avg_ar": compute_metric_averages dicts}."""
        if self._result is not None:
            return self._result
        dev = [(n, t) for n, (t, _, _) in self._scenes.items() if torch.is_tensor(t) and t.is_cuda]
        host_tables = {}
        if dev:                                  # one read-back for every device table
            flat = torch.cat([t.reshape(-1) for _, t in dev]).cpu().numpy()
            off = 0
            for n, t in dev:
                host_tables[n] = flat[off:off + t.numel()].reshape(t.shape)
                off += t.numel()
        scenes = []
        for n, (t, scores, classes) in self._scenes.items():
            t = host_tables.get(n, t)
            t = None if t is None else self._host(t).astype(np.int64)
            scenes.append(_scene_classes(t, self._gt[n][0], scores, classes, self.class_set, self.min_region_size))
        ap, ar = match_and_score(scenes, len(self.class_set.ids), self.min_region_size)
        names = self.class_set.names
        self._result = {"ap": ap, "ar": ar, "avg_ap": metric_averages(ap, names, "ap"),
                        "avg_ar": metric_averages(ar, names, "ar")}
        return self._result

    def result_rows(self):
        """The CSV rows of write_result_file (strings, header first)."""
        r = self.compute()
        rows = [["class", "class id", "ap", "ap50", "ap25", "ar", "ar50", "ar25"]]
        for name, cid in zip(self.class_set.names, self.class_set.ids):
            a, b = r["avg_ap"]["classes"][name], r["avg_ar"]["classes"][name]
            rows.append([str(x) for x in (name, cid, a["ap"], a["ap50%"], a["ap25%"], b["ar"], b["ar50%"],
                                          b["ar25%"])])
        return rows

    def write_result_file(self, path):
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        with open(path, "w") as f:
            for row in self.result_rows():
                f.write(",".join(row) + "\n")
