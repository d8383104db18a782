"""Reader of labelled scenes — the supervised counterpart of `FreeMaskSceneReader` (reference datasets/semseg.py:331-558,
the parts that are on in the shipped ScanNet config): `{scene}.npy` ([N,12]: xyz, rgb, normal, segment id, semantic
label, instance id) -> the 9-tuple (coordinates, features, labels [semantic, instance, segment], scene_name, raw_color,
raw_normals, raw_coordinates, idx, []) that `datasets.utils.VoxelizeCollate` takes.

Train mode runs the same augmentation as the FreeMask reader (datasets/augment.py, unchanged; same random draws in the
same order — the reference's two readers share that code line by line), validation mode only normalises the colours.
`_remap_from_zero` (:598-603) — every label that is no key of the label database becomes `ignore_label`, then key k
becomes its position i, one assignment after the other — is composed on the host into ONE lookup table, so a chain such
as 9 -> 0 -> 4 (keys [9, 4, 2, 1, 0]) comes out like the reference's in-place loop.

Not built (off in the shipped config, refused by the constructor): instance_oversampling, add_unlabeled_pc, cropping,
and what `FreeMaskSceneReader` already refuses (flip_in_center, point_per_cut, resample_points, noise_rate).  The label
database is a plain {id: {"validation": bool, ...}} mapping passed in."""
from __future__ import annotations

from random import sample

import numpy as np

from .freemask import SCANNET_COLOR_MEAN_STD, FreeMaskSceneReader


def select_labels(label_db, num_labels):
    """`_select_correct_labels` (:576-596): all labels, or the validation subset, by `num_labels`."""
    n_all = len(label_db)
    n_val = sum(1 for v in label_db.values() if v["validation"])
    if num_labels == n_all:
        return dict(label_db)
    if num_labels == n_val:
        return {k: v for k, v in label_db.items() if v["validation"]}
    raise ValueError(f"not available number labels, select from: {n_val}, {n_all}")


def remap_from_zero_table(keys, ignore_label=255):
    """i64 lookup table over 0 .. max(keys, ignore_label): the reference's sequential `_remap_from_zero` applied to
    every value at once.  Values outside the table are no keys: they map like `ignore_label` does."""
    keys = [int(k) for k in keys]
    lut = np.arange(max(keys + [int(ignore_label)]) + 1, dtype=np.int64)
    lut[~np.isin(lut, keys)] = ignore_label
    for i, k in enumerate(keys):
        lut[lut == k] = i
    return lut


def remap_from_zero(labels, lut, ignore_label=255):
    v = np.asarray(labels).astype(np.int64)
    inside = (v >= 0) & (v < lut.shape[0])
    return np.where(inside, lut[np.where(inside, v, 0)], lut[ignore_label])


class SupervisedSceneReader(FreeMaskSceneReader):
    """`SemanticSegmentationDataset.__getitem__` for dataset_name "scannet"; entries: dicts with "filepath" and
    "raw_filepath" (the database yaml), label_db: {label id: {"validation": bool, ...}} in the database's order."""

    def __init__(self, entries, label_db, num_labels=-1, color_mean_std=SCANNET_COLOR_MEAN_STD, mode="train",
                 add_colors=True, add_normals=True, add_raw_coordinates=False, add_instance=False, data_percent=1.0,
                 ignore_label=255, device="cuda", volume_augmentations=None, image_augmentations=None,
                 is_elastic_distortion=True, color_drop=0.0, instance_oversampling=0, add_unlabeled_pc=False,
                 cropping=False, flip_in_center=False, point_per_cut=0, resample_points=0, noise_rate=0):
        if instance_oversampling or add_unlabeled_pc or cropping:
            raise NotImplementedError("instance_oversampling / add_unlabeled_pc / cropping are off in the shipped ScanNet "
                                      "config (conf/data/datasets/scannet.yaml) and not built")
        super().__init__(entries, color_mean_std=color_mean_std, add_colors=add_colors, add_normals=add_normals,
                         add_raw_coordinates=add_raw_coordinates, device=device, mode=mode,
                         volume_augmentations=volume_augmentations, image_augmentations=image_augmentations,
                         is_elastic_distortion=is_elastic_distortion, flip_in_center=flip_in_center,
                         color_drop=color_drop, point_per_cut=point_per_cut, resample_points=resample_points,
                         noise_rate=noise_rate)
        if data_percent < 1.0:
            self.data = sample(self.data, int(len(self.data) * data_percent))
        self.add_instance, self.ignore_label = add_instance, ignore_label
        self.label_info = select_labels(label_db, num_labels)
        self.remap = remap_from_zero_table(self.label_info.keys(), ignore_label)

    def __getitem__(self, idx):
        idx = idx % len(self.data)
        points = np.load(self.data[idx]["filepath"].replace("../../", ""))
        coordinates, color, normals, segments, labels = (points[:, :3], points[:, 3:6], points[:, 6:9], points[:, 9],
                                                         points[:, 10:12])
        raw_coordinates, raw_color, raw_normals = coordinates.copy(), color, normals
        if not self.add_colors:
            color = np.ones((len(color), 3))
        labels = labels.astype(np.int32)
        if labels.size > 0:
            labels[:, 0] = remap_from_zero(labels[:, 0], self.remap, self.ignore_label)
            if not self.add_instance:
                labels = labels[:, 0].flatten()[..., None]     # the semantic label only
        name = self.data[idx]["raw_filepath"].split("/")[-2]
        if "train" in self.mode and hasattr(self.volume_augmentations, "transforms"):
            item = self._train_item(idx, coordinates, color, normals, segments, labels, raw_coordinates, raw_color,
                                    raw_normals)
            item = item[:3] + (name,) + item[4:]
        else:
            # albumentations.Normalize on the uint8-truncated colours (:519-520)
            features = (color.astype(np.uint8).astype(np.float32) - self.color_mean) * self.color_den
            if self.add_normals:
                features = np.hstack((features, normals))
            if self.add_raw_coordinates:
                features = np.hstack((features, coordinates))
            labels = np.hstack((labels, segments[..., None].astype(np.int32)))
            item = (coordinates, features, labels, name, raw_color, raw_normals, raw_coordinates, idx, [])
        if name in ("scene0636_00", "scene0154_00"):            # the two scenes the reference replaces by scene 0 (:542)
            return self[0]
        return item
