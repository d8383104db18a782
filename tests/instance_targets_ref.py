"""Numpy restatement of the reference's supervised collate targets (datasets/utils.py:235-368 `voxelize`, :529-613
`get_instance_masks`, task "instance_segmentation") — the oracle of the device path on a machine without the reference.
It imports nothing from the package; tests/golden/instance_targets.npz pins it to the reference's own outputs."""
import numpy as np


def instance_targets(labels, n_segments=None, filter_out_classes=(), label_offset=0):
    """One label table [N, >= 2(3)] -> (labels i64[T], masks bool[T,N], segment_mask bool[T,S] or None); T may be 0."""
    labels = np.asarray(labels).astype(np.int64)
    out_l, out_m, out_s = [], [], []
    for inst in np.unique(labels[:, 1]):               # ascending ids
        if inst == -1:
            continue
        rows = labels[:, 1] == inst
        label = labels[rows][0, 0]                     # the first row's label decides
        if int(label) in [int(c) for c in filter_out_classes]:
            continue
        # (reference :551: `255 in filter_out_classes and label == 255 and rows < ignore_class_threshold` can only hold
        #  for a label that the membership test above has already dropped)
        out_l.append(max(int(label) - label_offset, 0))
        out_m.append(rows)
        if n_segments is not None:
            sm = np.zeros(n_segments, bool)
            sm[labels[rows][:, 2]] = True
            out_s.append(sm)
    n = labels.shape[0]
    return (np.asarray(out_l, np.int64), np.asarray(out_m, bool).reshape(len(out_l), n),
            None if n_segments is None else np.asarray(out_s, bool).reshape(len(out_l), n_segments))


def get_instance_masks(list_labels, list_segments=None, filter_out_classes=(), label_offset=0):
    """The reference's list form: a scene without a kept instance makes the whole call return []."""
    target = []
    for b, table in enumerate(list_labels):
        S = None if not list_segments else len(list_segments[b])
        lab, masks, seg = instance_targets(table, S, filter_out_classes, label_offset)
        if lab.shape[0] == 0:
            return []
        entry = {"labels": lab, "masks": masks}
        if seg is not None:
            entry["segment_mask"] = seg
        target.append(entry)
    return target


def first_unique(keys):
    """Rows of the first occurrence of every distinct row of keys, in row order, and the inverse map (the rule of
    tests/test_host_voxelize.py for sparse_quantize)."""
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    return first[order], rank[inverse.reshape(-1)]


def voxelize(batch, voxel_size, mode, filter_out_classes=(), label_offset=0):
    """-> dict(coordinates i32[M,4], unique_maps, inverse_maps, target, target_full) for samples whose third item is an
    [N,3] label table; `mode` as in the reference ("train…", "validation", "test")."""
    coords, tables, umaps, imaps = [], [], [], []
    for sample in batch:
        c = np.floor(np.asarray(sample[0], dtype=np.float64) / voxel_size)
        um, im = first_unique(c.astype(np.int64))
        umaps.append(um)
        imaps.append(im)
        coords.append(c[um].astype(np.int32))
        tables.append(np.asarray(sample[2])[um].astype(np.int64))
    coordinates = np.concatenate([np.concatenate([np.full((len(c), 1), b, np.int32), c], 1) for b, c in enumerate(coords)])
    originals = [np.asarray(s[2]).astype(np.int64) for s in batch]
    target, target_full = [], []
    if mode == "test":
        for t, o in zip(tables, originals):
            t[:, 0] = np.unique(t[:, 0], return_inverse=True)[1].reshape(-1)
            target.append({"point2segment": t[:, 0].copy()})
            target_full.append({"point2segment": o[:, 0].copy()})
    else:
        seg2label = []
        for t in tables:
            _, index, inv = np.unique(t[:, -1], return_index=True, return_inverse=True)
            t[:, -1] = inv.reshape(-1)
            seg2label.append(t[index][:, :-1])
        target = get_instance_masks(tables, seg2label, filter_out_classes, label_offset)
        for i in range(len(target)):
            target[i]["point2segment"] = tables[i][:, 2].copy()
        if "train" not in mode:
            target_full = get_instance_masks(originals, None, filter_out_classes, label_offset)
            for i in range(len(target_full)):
                target_full[i]["point2segment"] = originals[i][:, 2].copy()
    return {"coordinates": coordinates, "unique_maps": umaps, "inverse_maps": imaps, "target": target,
            "target_full": target_full, "tables": tables}


def remap_table(keys, ignore_label=255, size=None):
    """`_remap_from_zero` (reference datasets/semseg.py:598-603) as ONE lookup table over the values 0..size-1: values
    that are no key become `ignore_label`, then the sequential `labels[labels == k] = i` assignments are applied in
    the reference's order (so an earlier result that equals a later key is remapped again, like the reference)."""
    keys = [int(k) for k in keys]
    size = max(max(keys, default=0), ignore_label) + 1 if size is None else size
    lut = np.arange(size, dtype=np.int64)
    lut[~np.isin(lut, keys)] = ignore_label
    for i, k in enumerate(keys):
        lut[lut == k] = i
    return lut
