"""Reader side of the self-training loop: the files the previous round exported
(`freemasks/{scene}_cloud.npy`, `{scene}_masks.npy`, written by trainer/postprocess.py::save_for_freemask) are merged
into a scene's pseudo masks, filtered, and turned into the 9-tuple the collate function takes.

Mirrors reference datasets/freemask_semseg.py — `load_self_train_masks` (:224-265) and `__getitem__` (:267-437) in
validation mode and in TRAIN mode: centring + random shift, axis flips, two elastic distortions, the volume and colour
augmentation pipelines, colour drop and normalisation run on the device (datasets/augment.py), drawing from numpy's and
python's global generators with the reference's own calls and in its order, so a seeded run consumes the same streams
(pinned by tests/golden/dataset.npz for the reference's own steps; the two third-party pipelines are restated from
their published definitions).  Random cuboid cuts / point resampling (point_per_cut, resample_points, noise_rate: 0 in
every shipped config) are not built.

The per-point work (1-NN transfer of the exported masks, the greedy merge, the extent filter) runs on the device.  With
`device_tables=True` the reader also builds the [N, K+2] mask table there (`mask_tables_device`, csrc/dataset.hip)
instead of with numpy on the host.  When the export wrote bit rows (`{scene}_masks_bits.npy`,
save_for_freemask(fmt="bits")), `load_self_train_bits` merges them with the kernels of csrc/selftrain.hip: one launch for
the greedy loop and one read-back (the number of added columns) instead of one per visited column.

`entries_from_database` / `load_color_mean_std` read what datasets/preprocessing.py writes."""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np
import torch

from .. import ops

SCANNET_COLOR_MEAN_STD = ((0.47793125906962, 0.4303257521323044, 0.3749598901421883),
                          (0.2834475483823543, 0.27566157565723015, 0.27018971370874995))


def load_self_train_masks(points, freemasks, self_train_cloud, self_train_masks, num_self_train_data=5,
                          drop_original=False, device="cuda"):
    """points [N,>=3] scene points, freemasks [N,K] the scene's pseudo masks; self_train_cloud [M,>=3] /
    self_train_masks bool[M,K'] the previous round's export, most confident first.
    -> freemasks with up to `num_self_train_data` new columns: an exported instance is added when more than half of
    it is not yet covered, and only its uncovered part is added (freemask_semseg.py:246-265).  Same dtype as the
    input, like the reference's np.concatenate."""
    dev = torch.device(device)
    xyz = torch.as_tensor(np.ascontiguousarray(np.asarray(points)[:, :3]), dtype=torch.float32, device=dev)
    cloud = torch.as_tensor(np.ascontiguousarray(np.asarray(self_train_cloud)[:, :3]), dtype=torch.float32, device=dev)
    st = torch.as_tensor(np.asarray(self_train_masks), device=dev).bool()
    same = xyz.shape[0] == cloud.shape[0] and bool(torch.isclose(xyz, cloud, rtol=1e-5, atol=1e-8).all())
    if not same:                                   # np.allclose(points[:, :3], cloud[:, :3]) failed: 1-NN transfer
        _, ind = ops.knn1(xyz.contiguous(), cloud.contiguous())
        st = st[ind]
    fm = np.asarray(freemasks)
    if drop_original:
        fm = np.zeros((fm.shape[0], 0), dtype=fm.dtype)
    fg = torch.as_tensor(fm, device=dev).bool().any(1) if fm.shape[1] else torch.zeros(xyz.shape[0], dtype=torch.bool,
                                                                                        device=dev)
    totals = st.sum(0).tolist()
    added, j = [], 0
    while len(added) < num_self_train_data and j < st.shape[1]:
        fresh = st[:, j] & ~fg
        # useful_iou = |new & ~foreground| / |new| > 0.5, in integers (an empty instance gives nan > 0.5 == False)
        if totals[j] > 0 and 2 * int(fresh.sum()) > totals[j]:
            added.append(fresh)
            fg = fg | fresh
        j += 1
    if not added:
        return fm
    new = torch.stack(added, 1).cpu().numpy()
    return np.concatenate([fm, new], axis=1)


def load_self_train_bits(points, freemasks, self_train_cloud, bits, num_self_train_data=5, drop_original=False,
                         device="cuda", as_device=False):
    """`load_self_train_masks` for the bit-row file (`{scene}_masks_bits.npy`, u64[K', ceil(M/64)], written by
    save_for_freemask(fmt="bits")): the same sameness test, then `ops.knn1` + `ops.mask_bits_gather` when the clouds
    differ; the covered points are `any(freemasks != 0)` packed as one bit row; the greedy loop is one
    `ops.selftrain_merge` launch, and the number of added columns is the only value read back.
    -> the array `load_self_train_masks` returns for the unpacked file (values and dtype).  `as_device`: that array as
    an f32 device tensor [N, K + added] which never visits the host (what `mask_tables_device` takes); the soft masks
    must then be f32, f16, bool or integer, as for `mask_tables_device`."""
    dev = torch.device(device)
    xyz = torch.as_tensor(np.ascontiguousarray(np.asarray(points)[:, :3]), dtype=torch.float32, device=dev)
    cloud = torch.as_tensor(np.ascontiguousarray(np.asarray(self_train_cloud)[:, :3]), dtype=torch.float32, device=dev)
    N, M = xyz.shape[0], cloud.shape[0]
    b = np.asarray(bits)
    if b.dtype != np.uint64 or b.ndim != 2 or b.shape[1] != (M + 63) // 64:
        raise ValueError(f"load_self_train_bits: bits must be uint64 [K', {(M + 63) // 64}] for a cloud of {M} points, "
                         f"got {b.dtype} {b.shape}")
    fm = np.asarray(freemasks)
    if as_device and fm.dtype != np.float32 and fm.dtype.kind not in "biu" and fm.dtype != np.float16:
        raise TypeError(f"load_self_train_bits: soft masks must be float32, bool or integer, got {fm.dtype}")
    if drop_original:
        fm = np.zeros((fm.shape[0], 0), dtype=fm.dtype)
    K = fm.shape[1]
    fm_d = torch.as_tensor(np.ascontiguousarray(fm), device=dev) if K and N else None
    added = 0
    if N and M and b.shape[0] and num_self_train_data > 0:
        st = torch.as_tensor(np.ascontiguousarray(b).view(np.int64), device=dev)
        same = N == M and bool(torch.isclose(xyz, cloud, rtol=1e-5, atol=1e-8).all())
        if same:
            total = ops.mask_bits_count(st, N)
        else:                                          # np.allclose failed: 1-NN transfer, on bit rows
            _, ind = ops.knn1(xyz.contiguous(), cloud.contiguous())
            st, total = ops.mask_bits_gather(st, M, ind, check_range=False)       # knn1 returns indices in [0, M)
        if fm_d is not None:
            fg = ops.mask_columns_to_bits((fm_d != 0).any(1).reshape(N, 1))[0][0].contiguous()
        else:
            fg = torch.zeros((N + 63) // 64, dtype=torch.int64, device=dev)
        fresh, picked, n_added = ops.selftrain_merge(st, total, N, fg, int(num_self_train_data))
        added = int(n_added)                           # the one read-back
    if not as_device:
        if not added:
            return fm
        new = ops.mask_bits_to_columns(fresh, N, rows=range(added), dtype=torch.bool).cpu().numpy()
        return np.concatenate([fm, new], axis=1)
    out = torch.empty((N, K + added), dtype=torch.float32, device=dev)
    if fm_d is not None:
        out[:, :K] = fm_d                              # exact: f32 as it is, bool / integer / f16 widened
    if added:
        ops.mask_bits_to_columns(fresh, N, rows=range(added), out=out, col0=K)
    return out


def filter_by_extent(coordinates, freemasks, hard_threshold=0.5, extent_max_ratio=0.8, device="cuda"):
    """Column indices of the masks that are non-empty and whose XY extent does not exceed `extent_max_ratio` of the
    scene's in either direction (freemask_semseg.py:300-310)."""
    dev = torch.device(device)
    c = torch.as_tensor(np.asarray(coordinates), device=dev)[:, :2]
    m = torch.as_tensor(np.asarray(freemasks), device=dev) > hard_threshold
    scene = (c.amax(0) - c.amin(0)) * extent_max_ratio
    inf = torch.finfo(c.dtype).max
    cc, mm = c[:, None, :], m[:, :, None]
    ext = torch.where(mm, cc, torch.full_like(cc, -inf)).amax(0) - torch.where(mm, cc, torch.full_like(cc, inf)).amin(0)
    keep = m.any(0) & ~(ext > scene).any(1)
    return keep.nonzero().flatten().tolist()


def mask_tables_device(coordinates, freemasks, segments, hard_threshold=0.5, extent_max_ratio=0.8, device="cuda"):
    """`filter_by_extent` and the table lines of `FreeMaskSceneReader.__getitem__` in two passes over the soft masks on
    the device, without the [N,K,2] temporaries: -> (table i32[N, len(keep)+2] on the device, keep).
    table[:, 0] = any kept mask set, table[:, 1:-1] = freemasks[:, keep] > threshold, table[:, -1] = (int32)segments;
    `keep` is `filter_by_extent`'s list.  With an empty `keep` the table is None.

    The threshold is rounded to f32 once, as numpy's `f32 array > python float` and torch's tensor-against-scalar
    comparison both do.  The keep decision is `filter_by_extent`'s f32 arithmetic on K-sized device vectors.  The soft
    masks must be f32, bool or integer (cast to f32 exactly); another float width would round differently from the
    host path and is refused.  `freemasks` may also be an f32 device tensor [N,K], which is used where it lies."""
    dev = torch.device(device)
    if torch.is_tensor(freemasks):                     # already on the device (load_self_train_bits(as_device=True))
        if freemasks.dtype != torch.float32 or not freemasks.is_cuda or freemasks.dim() != 2:
            raise TypeError("mask_tables_device: a tensor of soft masks must be float32 [N,K] on the device, got "
                            f"{freemasks.dtype} {tuple(freemasks.shape)} on {freemasks.device}")
        N, K = freemasks.shape
        if K == 0 or N == 0:
            return None, []
        soft = freemasks.contiguous()
    else:
        fm = np.asarray(freemasks)
        if fm.dtype != np.float32:
            if fm.dtype.kind not in "biu" and fm.dtype != np.float16:
                raise TypeError(f"mask_tables_device: soft masks must be float32, bool or integer, got {fm.dtype}")
            fm = fm.astype(np.float32)
        N, K = fm.shape
        if K == 0 or N == 0:
            return None, []
        soft = torch.as_tensor(np.ascontiguousarray(fm), device=dev)
    xyz_h = np.asarray(coordinates)[:, :3]
    if xyz_h.dtype != np.float32:
        raise TypeError(f"mask_tables_device: coordinates must be float32, got {xyz_h.dtype}")
    xyz = torch.as_tensor(np.ascontiguousarray(xyz_h), device=dev)
    count, lo, hi = ops.softmask_stats(soft, xyz, hard_threshold)
    c = xyz[:, :2]
    scene = (c.amax(0) - c.amin(0)) * extent_max_ratio
    keep = ((count > 0) & ~((hi - lo) > scene).any(1)).nonzero().flatten().tolist()
    if not keep:
        return None, keep
    seg = torch.as_tensor(np.ascontiguousarray(np.asarray(segments), dtype=np.float32), device=dev)
    return ops.softmask_table(soft, hard_threshold, keep, seg), keep


def entries_from_database(path):
    """`{mode}_database.yaml` (datasets/preprocessing.py; the reference's `_load_yaml`) -> the list of entry dicts the
    reader takes (`filepath`, `raw_filepath`, `scene`, `sub_scene`, `file_len`, `color_mean`, `color_std`, ...)."""
    import yaml

    with open(path) as f:
        entries = yaml.safe_load(f)
    if not isinstance(entries, list) or any(not isinstance(e, dict) or "filepath" not in e or "raw_filepath" not in e
                                            for e in entries):
        raise ValueError(f"{path}: not a scene database (a list of entries with filepath and raw_filepath)")
    return entries


def load_color_mean_std(path):
    """`color_mean_std.yaml` -> ((mean r, g, b), (std r, g, b)), the reader's `color_mean_std`."""
    import yaml

    with open(path) as f:
        d = yaml.safe_load(f)
    if not isinstance(d, dict) or len(d.get("mean", ())) != 3 or len(d.get("std", ())) != 3:
        raise ValueError(f"{path}: needs mean and std with three numbers each")
    return tuple(float(v) for v in d["mean"]), tuple(float(v) for v in d["std"])


class FreeMaskSceneReader:
    """Validation-mode `SemanticSegmentationFreeDataset.__getitem__`: `{scene}.npy` ([N,12]: xyz, rgb, normal,
    segment id, 2 unused) + `{scene}_freemasks.npy` ([N,K] soft masks) -> the 9-tuple
    (coordinates, features, freemasks+segments, scene_name, raw_color, raw_normals, raw_coordinates, idx, []).
    `resegment_mesh` (validation mode, both table paths): the segment column and the last field (int32[P,2] instead of
    []) come from the over-segmentation of the entry's mesh, see `segment_mesh`.
    `device_tables`: item 2 is built by `mask_tables_device` and returned as a device int32 tensor (the collate takes
    it as it is); same values, same random draws (the table path draws none)."""

    def __init__(self, entries, color_mean_std=SCANNET_COLOR_MEAN_STD, add_colors=True, add_normals=True,
                 add_raw_coordinates=False, freemask_hard_threshold=0.5, freemask_extent_max_ratio=0.8,
                 max_num_gt_instances=-1, load_self_train_data=False, self_train_data_dir=None, num_self_train_data=5,
                 device="cuda", mode="validation", volume_augmentations=None, image_augmentations=None,
                 is_elastic_distortion=True, flip_in_center=False, color_drop=0.0, point_per_cut=0, resample_points=0,
                 noise_rate=0, device_tables=False, resegment_mesh=False, segment_min_vert_num=20):
        self.data = list(entries)                      # dicts with "filepath" and "raw_filepath" (the database yaml)
        self.color_mean = np.asarray(color_mean_std[0], np.float32) * 255.0
        self.color_den = np.reciprocal(np.asarray(color_mean_std[1], np.float32) * 255.0)
        self.add_colors, self.add_normals, self.add_raw_coordinates = add_colors, add_normals, add_raw_coordinates
        self.freemask_hard_threshold = freemask_hard_threshold
        self.freemask_extent_max_ratio = freemask_extent_max_ratio
        self.max_num_gt_instances = max_num_gt_instances
        self.load_self_train_data = load_self_train_data
        self.self_train_data_dir = self_train_data_dir
        self.num_self_train_data = num_self_train_data
        self.device, self.device_tables = device, bool(device_tables)
        self.resegment_mesh, self.segment_min_vert_num = bool(resegment_mesh), int(segment_min_vert_num)
        self.mode, self.is_elastic_distortion, self.color_drop = mode, is_elastic_distortion, color_drop
        # objects with a `transforms` attribute, called like the reference's (volumentations / albumentations Compose);
        # datasets.augment.VolumeAugmentations() / ColorAugmentations() are the shipped YAML pipelines
        self.volume_augmentations, self.image_augmentations = volume_augmentations, image_augmentations
        if flip_in_center or point_per_cut or resample_points or noise_rate:
            raise NotImplementedError("flip_in_center / point_per_cut / resample_points / noise_rate are off in every "
                                      "shipped config (conf/data/datasets/*.yaml) and not built")

    def __len__(self):
        return len(self.data)

    def _self_train(self, idx, points, freemasks):
        scene_id = Path(self.data[idx]["filepath"]).stem
        name = "masks" if self.load_self_train_data != "refined" else "masks_refined"
        base = os.path.join(self.self_train_data_dir, "freemasks")
        bits_path = os.path.join(base, f"scene{scene_id}_masks_bits.npy")
        if name == "masks" and os.path.exists(bits_path):       # save_for_freemask(fmt="bits" | "both")
            try:
                cloud = np.load(os.path.join(base, f"scene{scene_id}_cloud.npy"))
            except FileNotFoundError:
                print(f"Could not load self training data for scene{scene_id}")
                return freemasks
            return load_self_train_bits(points, freemasks, cloud, np.load(bits_path), self.num_self_train_data,
                                        device=self.device, as_device=self.device_tables)
        try:
            cloud = np.load(os.path.join(base, f"scene{scene_id}_cloud.npy"))
            masks = np.load(os.path.join(base, f"scene{scene_id}_{name}.npy"))
        except FileNotFoundError:
            print(f"Could not load self training data for scene{scene_id}")
            return freemasks
        return load_self_train_masks(points, freemasks, cloud, masks, self.num_self_train_data, device=self.device)

    def __getitem__(self, idx):
        idx = idx % len(self.data)
        path = self.data[idx]["filepath"].replace("../../", "")
        points = np.load(path)
        freemasks = np.load(path.replace(".npy", "_freemasks.npy"))
        if self.load_self_train_data:
            freemasks = self._self_train(idx, points, freemasks)
        if self.max_num_gt_instances > 0:
            freemasks = freemasks[:, :self.max_num_gt_instances]
        coordinates, color, normals, segments = points[:, :3], points[:, 3:6], points[:, 6:9], points[:, 9]
        connectivity = []
        if self.resegment_mesh and "train" not in self.mode:        # freemask_semseg.py:302-303
            segments, connectivity = self.segment_mesh(idx, coordinates, segments)
        if self.device_tables:
            return self._item_device_tables(idx, path, coordinates, color, normals, segments, freemasks, connectivity)
        keep = filter_by_extent(coordinates, freemasks, self.freemask_hard_threshold, self.freemask_extent_max_ratio,
                                self.device)
        if not keep:
            raise LookupError(f"{path}: no usable pseudo mask")   # the reference resamples a random other scene
        freemasks = freemasks[:, keep]
        hard = freemasks > self.freemask_hard_threshold
        freemasks = np.concatenate([hard.any(1).astype(np.int32).reshape(-1, 1), hard.astype(np.int32)], axis=1)
        raw_coordinates, raw_color, raw_normals = coordinates.copy(), color, normals
        if not self.add_colors:
            color = np.ones((len(color), 3))
        if "train" in self.mode and hasattr(self.volume_augmentations, "transforms"):
            return self._train_item(idx, coordinates, color, normals, segments, freemasks, raw_coordinates, raw_color,
                                    raw_normals)
        # albumentations.Normalize on the uint8-truncated colours (freemask_semseg.py:408-409)
        features = (color.astype(np.uint8).astype(np.float32) - self.color_mean) * self.color_den
        if self.add_normals:
            features = np.hstack((features, normals))
        if self.add_raw_coordinates:
            features = np.hstack((features, coordinates))
        freemasks = np.hstack((freemasks, segments[..., None].astype(freemasks.dtype))).astype(np.int32)
        raw = self.data[idx]["raw_filepath"]
        scene_name = f"scene{raw.split('/')[-1].split('_')[0]}" if "arkit" in raw.lower() else raw.split("/")[-2]
        return coordinates, features, freemasks, scene_name, raw_color, raw_normals, raw_coordinates, idx, connectivity

    def segment_mesh(self, idx, coordinates, segments):
        """`resegment_mesh` (freemask_semseg.py:192-221): -> (segment id per point, connectivity int32[P,2]) from
        `felzenszwalb_cpp.segment_mesh(vertices, faces, colors, 0.005, segment_min_vert_num)` on the entry's
        `raw_filepath` mesh (numpy PLY reader); the ids go to the points through their exact nearest vertex when the
        counts differ.  An entry that names a `connectivity_filepath` written with the same `segments_min_verts`
        (datasets/preprocessing.py, write_connectivity) has that segmentation in its segment column already: the file
        is used and nothing is segmented.  An empty or unreadable mesh keeps the stored ids and gives [] with a message
        (the reference prints the same message and then fails on unpacking None)."""
        from .. import felzenszwalb_cpp
        from ..pseudo_masks import scans

        entry = self.data[idx]
        stored = entry.get("connectivity_filepath")
        if stored and int(entry.get("segments_min_verts", -1)) == self.segment_min_vert_num and os.path.exists(stored):
            return segments, np.load(stored).astype(np.int32).reshape(-1, 2)
        mesh_path = entry["raw_filepath"]
        try:
            vertices, colors, faces = scans.read_ply_mesh(mesh_path)
        except (OSError, ValueError) as e:
            print(f"Can't segment mesh at {mesh_path}: {e}")
            return segments, []
        if len(vertices) == 0:
            print(f"Can't segment mesh as it is empty at {mesh_path}")
            return segments, []
        dev = torch.device(self.device)
        seg, conn = felzenszwalb_cpp.segment_mesh(vertices, faces, colors, 0.005, self.segment_min_vert_num, device=dev)
        if coordinates.shape[0] != vertices.shape[0]:
            _, ind = ops.knn1(torch.as_tensor(np.ascontiguousarray(coordinates, dtype=np.float32), device=dev),
                              torch.as_tensor(np.ascontiguousarray(vertices, dtype=np.float32), device=dev))
            seg = seg[ind.cpu().numpy().reshape(-1)]
        return seg, conn

    def _item_device_tables(self, idx, path, coordinates, color, normals, segments, freemasks, connectivity):
        """`__getitem__` from the extent filter on, with the mask table built on the device, segment column included."""
        table, keep = mask_tables_device(coordinates, freemasks, segments, self.freemask_hard_threshold,
                                         self.freemask_extent_max_ratio, self.device)
        if not keep:
            raise LookupError(f"{path}: no usable pseudo mask")
        raw_coordinates, raw_color, raw_normals = coordinates.copy(), color, normals
        if not self.add_colors:
            color = np.ones((len(color), 3))
        if "train" in self.mode and hasattr(self.volume_augmentations, "transforms"):
            return self._train_item(idx, coordinates, color, normals, None, table, raw_coordinates, raw_color,
                                    raw_normals)
        features = (color.astype(np.uint8).astype(np.float32) - self.color_mean) * self.color_den
        if self.add_normals:
            features = np.hstack((features, normals))
        if self.add_raw_coordinates:
            features = np.hstack((features, coordinates))
        return (coordinates, features, table, self._scene_name(idx), raw_color, raw_normals, raw_coordinates, idx,
                connectivity)

    def _scene_name(self, idx):
        raw = self.data[idx]["raw_filepath"]
        return f"scene{raw.split('/')[-1].split('_')[0]}" if "arkit" in raw.lower() else raw.split("/")[-2]

    def _train_item(self, idx, coordinates, color, normals, segments, freemasks, raw_coordinates, raw_color, raw_normals):
        """freemask_semseg.py:333-437 with the per-point work on the device; coordinates / features come back as device
        tensors (the collate takes them as they are).  Random numbers: numpy's global generator for the shift and the
        elastic noise, python's `random` for the flips, the elastic gate and the colour drop — same calls, same order."""
        from random import random

        from . import augment as A

        dev = torch.device(self.device)
        c = torch.as_tensor(np.ascontiguousarray(coordinates), device=dev).contiguous()
        nrm = torch.as_tensor(np.ascontiguousarray(normals), device=dev).contiguous()
        col = torch.as_tensor(np.ascontiguousarray(color), dtype=torch.float32, device=dev).contiguous()
        A.center_and_shift(c)
        for i in (0, 1):
            if random() < 0.5:
                A.flip_axis(c, i)
        if random() < 0.95 and self.is_elastic_distortion:
            for granularity, magnitude in ((0.2, 0.4), (0.8, 1.6)):
                A.elastic_distortion(c, granularity, magnitude)
        aug = self.volume_augmentations(points=c, normals=nrm, features=col, labels=freemasks)
        c, col, nrm, freemasks = aug["points"], aug["features"], aug["normals"], aug["labels"]
        tables = self.image_augmentations.tables() if self.image_augmentations is not None else None
        if random() < self.color_drop:
            tables = np.full((3, 256), 255, np.uint8)                  # color[:] = 255
        features = A.color_tables_to_features(col, tables, self.color_mean, self.color_den)
        if self.add_normals:
            features = torch.cat([features, nrm.to(features.dtype)], 1)
        if self.add_raw_coordinates:
            features = torch.cat([features, c.to(features.dtype)], 1)
        if segments is not None:                       # device tables carry the segment column already
            freemasks = np.hstack((freemasks, segments[..., None].astype(freemasks.dtype))).astype(np.int32)
        return c, features, freemasks, self._scene_name(idx), raw_color, raw_normals, raw_coordinates, idx, []
