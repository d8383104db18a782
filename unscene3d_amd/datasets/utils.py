"""Collate for the self-training path (reference datasets/utils.py:181-219, :370-527, :670-687):
`FreeMaskVoxelizeCollate` / `freemask_voxelize` turn a list of dataset 9-tuples
(coordinates, features, freemasks[labels | K mask columns | segment id], scene, raw_color, raw_normals,
raw_coordinates, idx, segment_connectivity — reference datasets/freemask_semseg.py:434) into
(NoGpu(coordinates i32[N,4], features f32[N,C], …), targets, scene names).

MI355X differences: the 2 cm voxelisation (`np.floor(xyz/voxel)` + ME.utils.sparse_quantize, reference
:403-408) runs on the device through the hash-unique kernel instead of in CPU DataLoader workers, and
the voxel rows may optionally be re-ordered into z-order cells (`spatial_sort`: True = 8^3-voxel cells, or the cell
size as a power of two, e.g. 5 = 32^3 voxels), a consistent permutation of every per-voxel array (inverse maps are
remapped accordingly)."""
from __future__ import annotations

import numpy as np
import torch

from .. import MinkowskiEngine as ME
from .. import ops


def _dev(x, dev, dtype):
    """numpy array or tensor (possibly already resident in HBM) -> contiguous device tensor."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=dev, dtype=dtype).contiguous()


class NoGpu:
    """Plain container (reference :670-687)."""

    def __init__(self, coordinates, features, original_labels=None, inverse_maps=None, full_res_coords=None,
                 target_full=None, original_colors=None, original_normals=None, original_coordinates=None, idx=None,
                 segment_connectivity=None):
        self.coordinates, self.features = coordinates, features
        self.original_labels, self.inverse_maps, self.full_res_coords = original_labels, inverse_maps, full_res_coords
        self.target_full, self.original_colors, self.original_normals = target_full, original_colors, original_normals
        self.original_coordinates, self.idx, self.segment_connectivity = original_coordinates, idx, segment_connectivity


def get_instance_freemasks(list_freemasks, list_segments=None):
    """Targets from [labels | K mask columns | segment id] tables (reference :480-527).

    Every non-empty mask column becomes one foreground target (label 1).  With segments, the segment
    mask of a target is set at `unique(ALL values of the rows inside the mask)` — the reference takes
    the unique over whole table rows (label column and the 0/1 mask values included, :503), which is
    reproduced here.  Vectorised over the K columns (one host sync per scene instead of K)."""
    target = []
    for b, table in enumerate(list_freemasks):
        colsT = (table[:, 1:-1] != 0).T.contiguous()                # [K, N] hard masks (row reductions are fast)
        keep = torch.nonzero(colsT.any(1)).reshape(-1)              # non-empty columns (host sync)
        if keep.numel() == 0:
            return []
        masks = colsT[keep]                                         # [T, N]
        entry = {"labels": torch.ones(keep.numel(), dtype=torch.int64, device=table.device), "masks": masks}
        if list_segments:
            S = list_segments[b].shape[0]
            tt, rr = torch.nonzero(masks, as_tuple=True)            # (target, row) pairs
            vals = table[rr]                                        # [P, K+2] every value of those rows
            sm = torch.zeros((keep.numel(), S), dtype=torch.bool, device=table.device)
            sm[tt[:, None].expand_as(vals).reshape(-1), vals.reshape(-1)] = True
            entry["segment_mask"] = sm
        target.append(entry)
    return target


def freemask_voxelize(batch, ignore_label, voxel_size, mode, ignore_class_threshold, device="cuda",
                      spatial_sort=False):
    dev = torch.device(device)
    coords_l, feats_l, tables, inverse_maps = [], [], [], []
    full_res_coords, original_freemasks, colors, normals, raw_coords, idx, seg_conn = [], [], [], [], [], [], []
    for sample in batch:
        full_res_coords.append(sample[0])
        original_freemasks.append(sample[2])
        colors.append(sample[4])
        normals.append(sample[5])
        raw_coords.append(sample[6])
        idx.append(sample[7])
        seg_conn.append(sample[8])
        xyz = _dev(sample[0], dev, torch.float64)
        c3, unique_map, inverse_map = ME.utils.sparse_quantize(xyz, quantization_size=voxel_size, return_index=True,
                                                               return_inverse=True, device=str(dev))
        if spatial_sort:
            c4 = torch.cat([torch.zeros((c3.shape[0], 1), dtype=torch.int32, device=dev), c3], 1).contiguous()
            order = ops.spatial_order(c4, shift=int(spatial_sort) if spatial_sort is not True else 3)
            rank = torch.empty_like(order)
            rank[order] = torch.arange(order.shape[0], device=dev)
            c3, unique_map, inverse_map = c3[order], unique_map[order], rank[inverse_map]
        inverse_maps.append(inverse_map)
        coords_l.append(c3.int())
        feats_l.append(_dev(sample[1], dev, torch.float32)[unique_map])
        if len(sample[2]) > 0:
            tables.append(_dev(sample[2], dev, torch.int64)[unique_map])

    if tables:   # pad the mask columns to a common width, keeping the segment id as the last column
        width = max(t.shape[1] for t in tables)
        tables = [torch.cat([t[:, :-1], t.new_zeros(t.shape[0], width - t.shape[1]), t[:, -1:]], dim=1) for t in tables]
        coordinates, features, _ = ME.utils.sparse_collate(coords_l, feats_l, tables)
    else:
        coordinates, features = ME.utils.sparse_collate(coords_l, feats_l)

    target, target_full = [], []
    if tables:
        segment2label, n_segments = [], []
        for t in tables:
            seg = t[:, -1]
            uniq, inv = torch.unique(seg, return_inverse=True)
            n_segments.append(int(uniq.shape[0]))           # known on the host here: saves the model a read-back
            first = torch.full((uniq.shape[0],), seg.shape[0], dtype=torch.long, device=dev)
            first.scatter_reduce_(0, inv, torch.arange(seg.shape[0], device=dev), reduce="amin")
            t[:, -1] = inv                                   # contiguous segment ids (np.unique return_inverse)
            segment2label.append(t[first][:, :-1])
        target = get_instance_freemasks(tables, list_segments=segment2label)
        for i in range(len(target)):
            target[i]["point2segment"] = tables[i][:, -1].contiguous()   # a row-gather index: the kernels take dense i64
            target[i]["num_segments"] = torch.tensor(n_segments[i])     # host scalar (a tensor like the other entries)
        full = [m if isinstance(m, torch.Tensor) else torch.as_tensor(np.asarray(m)) for m in original_freemasks]
        target_full = get_instance_freemasks(full)
        for i in range(len(target_full)):
            target_full[i]["point2segment"] = full[i][:, -1].long()
    else:
        coordinates, features = [], []
    return (NoGpu(coordinates, features, original_freemasks, inverse_maps, full_res_coords, target_full, colors,
                  normals, raw_coords, idx, seg_conn), target, [sample[3] for sample in batch])


class FreeMaskVoxelizeCollate:
    def __init__(self, ignore_label=255, voxel_size=1, mode="test", small_crops=False, very_small_crops=False,
                 batch_instance=False, probing=False, task="instance_segmentation", ignore_class_threshold=100,
                 filter_out_classes=(), label_offset=0, num_queries=None, device="cuda", spatial_sort=False):
        assert task in ["instance_segmentation"], "task not known"
        if small_crops or very_small_crops:
            raise NotImplementedError("crop collates are outside the accelerated path (SURVEY.md §2.1)")
        self.ignore_label, self.voxel_size, self.mode = ignore_label, voxel_size, mode
        self.ignore_class_threshold, self.device, self.spatial_sort = ignore_class_threshold, device, spatial_sort

    def __call__(self, batch):
        return freemask_voxelize(batch, self.ignore_label, self.voxel_size, self.mode, self.ignore_class_threshold,
                                 device=self.device, spatial_sort=self.spatial_sort)


# ---------------------------------------------------------------------------------------------------------------------
# The supervised path (reference :6-45 VoxelizeCollate, :235-368 voxelize, :529-613 get_instance_masks): ground-truth
# [semantic label, instance id, segment id] tables instead of pseudo-mask columns.
def get_instance_masks(list_labels, task, list_segments=None, ignore_class_threshold=100, filter_out_classes=(),
                       label_offset=0):
    """Targets from [semantic label, instance id(, segment id)] tables (reference :529-613) -> a list of
    {"labels" i64[T], "masks" bool[T,N][, "segment_mask" bool[T,S]]}, one per table, built by `ops.instance_targets`
    (csrc/targets.hip) instead of the reference's loop over instances: one target per instance id other than -1, in
    ascending id order, whose label — column 0 of the instance's FIRST row — is not in `filter_out_classes`;
    labels = clamp(label - label_offset, min=0).  With `list_segments` (the segment2label tables; only their lengths
    are used) column 2 holds segment ids in [0, len(list_segments[b])).

    Reference quirks kept: a table without a kept instance makes the WHOLE call return [] (:562-563).
    `ignore_class_threshold` is accepted and has no effect: the reference applies it only when 255 is in
    `filter_out_classes` and the label is 255 (:551), and the membership test in front of it (:548) has then already
    dropped the instance — the rule can never fire, with any threshold.
    One device->host read per table (the number of targets, for the allocation), like get_instance_freemasks."""
    if task == "semantic_segmentation":
        raise NotImplementedError("task='semantic_segmentation' targets are outside the accelerated path (SURVEY.md §2.1)")
    target = []
    for b, table in enumerate(list_labels):
        table = _dev(table, table.device if isinstance(table, torch.Tensor) and table.is_cuda else "cuda", torch.int64)
        n_seg = list_segments[b].shape[0] if list_segments else None
        labels, masks, segment_mask = ops.instance_targets(table, n_seg, filter_out_classes, label_offset)
        if labels.shape[0] == 0:
            return []
        entry = {"labels": labels, "masks": masks}
        if segment_mask is not None:
            entry["segment_mask"] = segment_mask
        target.append(entry)
    return target


def voxelize(batch, ignore_label, voxel_size, probing, mode, task, ignore_class_threshold, filter_out_classes,
             label_offset, num_queries, device="cuda", spatial_sort=False):
    """The supervised collate (reference :235-368) on the device, like `freemask_voxelize`: a list of dataset tuples
    (coordinates, features, labels [N,3] = [semantic, instance, segment], scene, raw_color, raw_normals,
    raw_coordinates, idx[, segment_connectivity]) -> (NoGpu, targets, scene names).

    Train / validation: the segment ids are renumbered through unique-inverse, `segment2label` is built from the first
    row of every segment, the targets come from `get_instance_masks` and every target also carries `point2segment` and
    `num_segments` (a host scalar, as in the FreeMask path).  Non-train modes build `target_full` from the
    full-resolution tables.  mode == "test": column 0 is renumbered and the targets carry `point2segment` only (in
    `target` and `target_full`).  1-D label tables take the reference's `labels == label_ids.unsqueeze(1)` branch (255
    dropped; the reference's segment renumbering would fail on them and is skipped).  `probing` returns
    (NoGpu(coordinates, features, original_labels, inverse_maps), labels) early.

    `spatial_sort` permutes every per-voxel array consistently (coordinates, features, label rows; the inverse maps are
    remapped).  The first-row rule of an instance's label and of `segment2label` then refers to the rows AS EMITTED,
    i.e. to the sorted order."""
    dev = torch.device(device)
    coords_l, feats_l, tables, inverse_maps = [], [], [], []
    full_res_coords, original_labels, colors, normals, raw_coords, idx = [], [], [], [], [], []
    for sample in batch:
        idx.append(sample[7])
        raw_coords.append(sample[6])
        original_labels.append(sample[2])
        full_res_coords.append(sample[0])
        colors.append(sample[4])
        normals.append(sample[5])
        xyz = _dev(sample[0], dev, torch.float64)
        c3, unique_map, inverse_map = ME.utils.sparse_quantize(xyz, quantization_size=voxel_size, return_index=True,
                                                               return_inverse=True, device=str(dev))
        if spatial_sort:
            c4 = torch.cat([torch.zeros((c3.shape[0], 1), dtype=torch.int32, device=dev), c3], 1).contiguous()
            order = ops.spatial_order(c4, shift=int(spatial_sort) if spatial_sort is not True else 3)
            rank = torch.empty_like(order)
            rank[order] = torch.arange(order.shape[0], device=dev)
            c3, unique_map, inverse_map = c3[order], unique_map[order], rank[inverse_map]
        inverse_maps.append(inverse_map)
        coords_l.append(c3.int())
        feats_l.append(_dev(sample[1], dev, torch.float32)[unique_map])
        if len(sample[2]) > 0:
            tables.append(_dev(sample[2], dev, torch.int64)[unique_map])

    if tables:
        coordinates, features, labels = ME.utils.sparse_collate(coords_l, feats_l, tables)
    else:
        coordinates, features = ME.utils.sparse_collate(coords_l, feats_l)
        labels = torch.Tensor([])
    if probing:
        return NoGpu(coordinates, features, original_labels, inverse_maps), labels

    def full_table(x):
        return _dev(x, dev, torch.int64)

    target, target_full = [], []
    if tables and tables[0].dim() == 1:
        for t in tables:
            label_ids = t.unique()
            if bool((label_ids == 255).any()):
                label_ids = label_ids[:-1]
            target.append({"labels": label_ids, "masks": t == label_ids.unsqueeze(1)})
    elif tables:
        column = 0 if mode == "test" else -1
        n_groups, first_rows = [], []
        for t in tables:                                     # contiguous ids (np.unique return_inverse), :298 / :306
            uniq, inv = torch.unique(t[:, column], return_inverse=True)
            n_groups.append(int(uniq.shape[0]))
            first = torch.full((uniq.shape[0],), t.shape[0], dtype=torch.long, device=dev)
            first.scatter_reduce_(0, inv, torch.arange(t.shape[0], device=dev), reduce="amin")
            first_rows.append(first)
            t[:, column] = inv
        if mode == "test":
            for i, t in enumerate(tables):
                target.append({"point2segment": t[:, 0].contiguous(), "num_segments": torch.tensor(n_groups[i])})
                target_full.append({"point2segment": full_table(original_labels[i])[:, 0].contiguous()})
        else:
            segment2label = [t[f][:, :-1] for t, f in zip(tables, first_rows)]       # [label, instance id]
            target = get_instance_masks(tables, task, list_segments=segment2label,
                                        ignore_class_threshold=ignore_class_threshold,
                                        filter_out_classes=filter_out_classes, label_offset=label_offset)
            for i in range(len(target)):
                target[i]["point2segment"] = tables[i][:, 2].contiguous()
                target[i]["num_segments"] = torch.tensor(n_groups[i])
            if "train" not in mode:
                full = [full_table(l) for l in original_labels]
                target_full = get_instance_masks(full, task, ignore_class_threshold=ignore_class_threshold,
                                                 filter_out_classes=filter_out_classes, label_offset=label_offset)
                for i in range(len(target_full)):
                    target_full[i]["point2segment"] = full[i][:, 2].contiguous()
    else:
        coordinates, features = [], []
    names = [sample[3] for sample in batch]
    if "train" not in mode:
        return (NoGpu(coordinates, features, original_labels, inverse_maps, full_res_coords, target_full, colors,
                      normals, raw_coords, idx), target, names)
    return NoGpu(coordinates, features, original_labels, inverse_maps, full_res_coords), target, names


class VoxelizeCollate:
    """The reference's default collation (`voxelize_collate`, :6-45) with `device` and `spatial_sort` added."""

    def __init__(self, ignore_label=255, voxel_size=1, mode="test", small_crops=False, very_small_crops=False,
                 batch_instance=False, probing=False, task="instance_segmentation", ignore_class_threshold=100,
                 filter_out_classes=(), label_offset=0, num_queries=None, device="cuda", spatial_sort=False):
        assert task in ["instance_segmentation", "semantic_segmentation"], "task not known"
        if small_crops or very_small_crops:
            raise NotImplementedError("crop collates are outside the accelerated path (SURVEY.md §2.1)")
        if batch_instance:
            raise NotImplementedError("batch_instance is outside the accelerated path (SURVEY.md §2.1)")
        self.task, self.filter_out_classes, self.label_offset = task, filter_out_classes, label_offset
        self.ignore_label, self.voxel_size, self.mode, self.probing = ignore_label, voxel_size, mode, probing
        self.ignore_class_threshold, self.num_queries = ignore_class_threshold, num_queries
        self.device, self.spatial_sort = device, spatial_sort

    def __call__(self, batch):
        return voxelize(batch, self.ignore_label, self.voxel_size, self.probing, self.mode, task=self.task,
                        ignore_class_threshold=self.ignore_class_threshold, filter_out_classes=self.filter_out_classes,
                        label_offset=self.label_offset, num_queries=self.num_queries, device=self.device,
                        spatial_sort=self.spatial_sort)
