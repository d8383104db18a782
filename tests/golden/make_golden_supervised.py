#!/usr/bin/env python
"""Golden-vector generator for the supervised collate — runs ONLY where /root/reference exists (like make_golden.py).
Imports the reference's datasets/utils.py in place with a stub `MinkowskiEngine` module (sparse_quantize = the
first-occurrence numpy unique of tests/test_host_voxelize.py, sparse_collate = batch column + concatenate), runs
`get_instance_masks` on constructed label tables and `voxelize` on one two-scene ragged batch in train, validation and
test mode, and stores inputs and outputs in tests/golden/instance_targets.npz (masks bit-packed).  It also stores label
vectors with the reference's sequential `_remap_from_zero` applied.  Nothing of the reference is copied; the fixture
is data.

    python tests/golden/make_golden_supervised.py

get_instance_masks cases (tables [semantic label, instance id, segment id]):
    basic         5 000 rows, gapped ids not in row order, some rows -1, filter [0, 1], label_offset 2, segments
    two_labels    instances whose rows carry two labels: the FIRST row decides (one kept, one dropped by it)
    interleaved   two instances alternating row by row, no segments
    all_filtered  every class filtered -> the call returns []
    offset_clamp  label_offset larger than some labels -> 0
    wide_ids      ids negative, gapped and >= 2^31
    ignore_255    255 in filter_out_classes with a small 255 instance and ignore_class_threshold (the rule that cannot fire)
    two_scenes    a list of two tables
    second_empty  a list whose second table keeps nothing -> [] for the whole call
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "instance_targets.npz")
MODES = ("train", "validation", "test")


def first_unique(keys):
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    return first[order], rank[inverse.reshape(-1)]


def import_reference_utils():
    me = types.ModuleType("MinkowskiEngine")
    me.utils = types.ModuleType("MinkowskiEngine.utils")

    def sparse_quantize(coordinates, features=None, ignore_label=None, return_index=False, return_inverse=False):
        um, im = first_unique(coordinates.numpy().astype(np.int64))
        return None, None, torch.from_numpy(um), torch.from_numpy(im)

    def sparse_collate(coords, feats, labels=None):
        c = torch.cat([torch.cat([torch.full((len(x), 1), b, dtype=torch.int32), x.int()], 1) for b, x in enumerate(coords)])
        f = torch.cat(feats)
        return (c, f) if labels is None else (c, f, torch.cat(labels))

    me.utils.sparse_quantize, me.utils.sparse_collate = sparse_quantize, sparse_collate
    sys.modules["MinkowskiEngine"], sys.modules["MinkowskiEngine.utils"] = me, me.utils
    sys.path.insert(0, REF)
    return importlib.import_module("datasets.utils")


def table(rng, n, ids, labels_of, n_seg, unlabeled=0.05):
    """Rows in random order: instance ids from `ids` (label labels_of[id]), a few rows -1, segment ids with gaps."""
    inst = rng.choice(np.asarray(ids, np.int64), n)
    lab = np.asarray([labels_of[int(i)] for i in inst], np.int64)
    drop = rng.random(n) < unlabeled
    inst[drop] = -1
    seg = rng.integers(0, n_seg, n) * 3 + 7
    return np.stack([lab, inst, seg], 1).astype(np.int64)


def cases():
    rng = np.random.default_rng(20240)
    out = {}
    ids = [40, 3, 17, 1001, 5, 260, 8, 90]
    labs = dict(zip(ids, [18, 0, 5, 5, 1, 2, 2, 5]))
    out["basic"] = dict(tables=[table(rng, 5000, ids, labs, 300)], segments=True, filter=[0, 1], offset=2)
    t = table(rng, 400, [4, 9, 12], {4: 3, 9: 6, 12: 1}, 40, unlabeled=0.0)
    r4, r9 = np.nonzero(t[:, 1] == 4)[0], np.nonzero(t[:, 1] == 9)[0]
    t[r4[0], 0], t[r4[1:], 0] = 1, 3          # first row filtered, the others not -> dropped
    t[r9[0], 0], t[r9[1:], 0] = 6, 0          # first row kept, the others filtered -> kept with label 6
    out["two_labels"] = dict(tables=[t], segments=True, filter=[0, 1], offset=0)
    t = np.zeros((129, 3), np.int64)
    t[:, 1] = np.where(np.arange(129) % 2 == 0, 70, 21)
    t[:, 0] = np.where(np.arange(129) % 2 == 0, 4, 9)
    out["interleaved"] = dict(tables=[t[:, :2].copy()], segments=False, filter=[], offset=0)
    out["all_filtered"] = dict(tables=[table(rng, 300, [1, 2, 3], {1: 0, 2: 1, 3: 0}, 20)], segments=True,
                               filter=[0, 1], offset=2)
    out["offset_clamp"] = dict(tables=[table(rng, 300, [1, 2, 3, 4], {1: 0, 2: 1, 3: 7, 4: 2}, 20)], segments=True,
                               filter=[], offset=2)
    wide = [-(2 ** 40), -7, 0, 2 ** 31, 2 ** 31 + 5, 2 ** 62]
    out["wide_ids"] = dict(tables=[table(rng, 700, wide, dict(zip(wide, [2, 3, 4, 5, 6, 7])), 64)], segments=True,
                           filter=[3], offset=1)
    t = table(rng, 900, [10, 20, 30], {10: 255, 20: 4, 30: 255}, 50)
    t = t[~((t[:, 1] == 30) & (rng.random(900) < 0.9))]          # a small 255 instance (< threshold rows)
    out["ignore_255"] = dict(tables=[t], segments=True, filter=[0, 1, 255], offset=2, threshold=100)
    out["two_scenes"] = dict(tables=[table(rng, 500, ids, labs, 60), table(rng, 333, [2, 6], {2: 7, 6: 3}, 31)],
                             segments=True, filter=[0, 1], offset=2)
    out["second_empty"] = dict(tables=[table(rng, 200, [2, 6], {2: 7, 6: 3}, 31), table(rng, 100, [5], {5: 1}, 9)],
                               segments=True, filter=[0, 1], offset=2)
    return out


def pack(z, key, m):
    m = m.numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
    z[key + "/shape"] = np.asarray(m.shape, np.int64)
    z[key + "/bits"] = np.packbits(m.astype(bool).reshape(-1))


def store_targets(z, key, target):
    z[key + "/count"] = np.asarray(len(target), np.int64)
    for b, t in enumerate(target):
        for name, v in t.items():
            if name in ("masks", "segment_mask"):
                pack(z, f"{key}/{b}/{name}", v)
            else:
                z[f"{key}/{b}/{name}"] = v.numpy().astype(np.int64)


def scene(rng, n, ids, labs, n_seg, box):
    xyz = rng.uniform(0, box, (n, 3))
    t = table(rng, n, ids, labs, n_seg).astype(np.int32)
    feats = rng.normal(size=(n, 6)).astype(np.float16).astype(np.float32)
    return (xyz, feats, t, f"scene{n:04d}_00", feats[:, :3].copy(), feats[:, 3:].copy(), xyz.astype(np.float32), n)


def main():
    U = import_reference_utils()
    z = {}
    names = []
    for name, c in cases().items():
        names.append(name)
        tables = [torch.from_numpy(t.copy()) for t in c["tables"]]
        seg2label = None
        if c["segments"]:                         # what the reference's voxelize does in front of the call (:306-308)
            seg2label = []
            for t in tables:
                _, idx, inv = np.unique(t[:, -1], return_index=True, return_inverse=True)
                t[:, -1] = torch.from_numpy(inv.reshape(-1))
                seg2label.append(t[idx][:, :-1])
        target = U.get_instance_masks(tables, "instance_segmentation", list_segments=seg2label,
                                      ignore_class_threshold=c.get("threshold", 100), filter_out_classes=c["filter"],
                                      label_offset=c["offset"])
        z[f"case/{name}/n_tables"] = np.asarray(len(tables), np.int64)
        for b, t in enumerate(tables):
            z[f"case/{name}/table{b}"] = t.numpy()
            z[f"case/{name}/n_segments{b}"] = np.asarray(len(seg2label[b]) if seg2label else -1, np.int64)
        z[f"case/{name}/filter"] = np.asarray(c["filter"], np.int64)
        z[f"case/{name}/offset"] = np.asarray(c["offset"], np.int64)
        z[f"case/{name}/threshold"] = np.asarray(c.get("threshold", 100), np.int64)
        store_targets(z, f"case/{name}/target", target)
    z["case_names"] = np.asarray(names)

    # ---- voxelize: one ragged two-scene batch, three modes
    rng = np.random.default_rng(777)
    ids = [40, 3, 17, 1001, 5, 260, 8, 90]
    labs = dict(zip(ids, [18, 0, 5, 5, 1, 2, 2, 5]))
    batch = [scene(rng, 2600, ids, labs, 90, 0.5), scene(rng, 1500, [2, 6, 11], {2: 7, 6: 3, 11: 1}, 40, 0.36)]
    for b, s in enumerate(batch):
        z[f"vox/scene{b}/xyz"], z[f"vox/scene{b}/feats"], z[f"vox/scene{b}/labels"] = s[0], s[1], s[2]
    z["vox/voxel_size"] = np.asarray(0.05)
    z["vox/filter"], z["vox/offset"] = np.asarray([0, 1], np.int64), np.asarray(2, np.int64)
    for mode in MODES:
        fresh = [tuple(x.copy() if isinstance(x, np.ndarray) else x for x in s) for s in batch]
        data, target, names_ = U.voxelize(fresh, 255, 0.05, False, mode, task="instance_segmentation",
                                          ignore_class_threshold=100, filter_out_classes=[0, 1], label_offset=2,
                                          num_queries=None)
        z[f"vox/{mode}/coordinates"] = data.coordinates.numpy().astype(np.int32)
        for b, im in enumerate(data.inverse_maps):
            z[f"vox/{mode}/inverse_map{b}"] = im.numpy().astype(np.int64)
        store_targets(z, f"vox/{mode}/target", target)
        store_targets(z, f"vox/{mode}/target_full", data.target_full or [])

    # ---- _remap_from_zero: the reference's sequential assignments on stored vectors
    for missing in ("albumentations", "volumentations", "yaml", "scipy"):   # third-party imports the remap never uses
        try:
            importlib.import_module(missing)
        except ImportError:
            sys.modules[missing] = types.ModuleType(missing)
    sem = importlib.import_module("datasets.semseg").SemanticSegmentationDataset
    rng = np.random.default_rng(5)
    key_sets = {"scannet20": [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39],
                "descending": [9, 4, 2, 1, 0], "with_255": [3, 255, 1, 2]}
    for name, keys in key_sets.items():
        holder = types.SimpleNamespace(label_info={k: {} for k in keys}, ignore_label=255)
        v = rng.integers(0, 300, 400).astype(np.int32)
        z[f"remap/{name}/keys"] = np.asarray(keys, np.int64)
        z[f"remap/{name}/in"] = v.copy()
        z[f"remap/{name}/out"] = sem._remap_from_zero(holder, v.copy())
    z["remap_names"] = np.asarray(list(key_sets))

    np.savez_compressed(OUT, **z)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(z)} arrays")


if __name__ == "__main__":
    main()
