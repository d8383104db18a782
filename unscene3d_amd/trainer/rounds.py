"""Between two self-training rounds (reference scripts/mask3d_DINO_CSC_self_train.sh: four rounds; after each one
every training scene goes through `eval_instance_step` with `general.save_for_freemask`): `export_round` runs
`InstanceSegmentation.eval_step` over a dataset and leaves the directory the next round's reader merges
(`FreeMaskSceneReader(load_self_train_data=True, self_train_data_dir=out_dir)`, tools/train.py --self-train-dir)."""
from __future__ import annotations

import copy
import os
from pathlib import Path

import torch

from ..config import apply_overrides

_SUFFIXES = {"npy": ("_cloud.npy", "_masks.npy"), "bits": ("_cloud.npy", "_masks_bits.npy"),
             "both": ("_cloud.npy", "_masks.npy", "_masks_bits.npy")}


def export_name(scenes, i, item):
    """The file stem of scene i: `scene{stem of the entry's filepath}`, the name `FreeMaskSceneReader._self_train`
    looks for; for the ScanNet layout this is also the reader's scene name (item[3]).  A plain list of items has no
    database entries and gives item[3]."""
    data = getattr(scenes, "data", None)
    if data is not None and "filepath" in data[i % len(data)]:
        return f"scene{Path(data[i % len(data)]['filepath']).stem}"
    return item[3]


def load_round_weights(module, path):
    """The weights of a `TrainLoop` checkpoint (or of a reference-format {"state_dict": ...}) into `module`."""
    state = torch.load(path, map_location="cpu", weights_only=False)
    res = module.load_state_dict(state["state_dict"], strict=False)
    bad = [k for k in list(res.missing_keys) + list(res.unexpected_keys) if k.startswith("model.")]
    if bad:
        raise RuntimeError(f"load_round_weights: model keys do not match {path}: {bad[:6]}")
    return state


def export_round(module, cfg, scenes, out_dir, *, fmt="npy", device, overrides=()):
    """One `eval_step` per scene of `scenes` (a validation-mode `FreeMaskSceneReader`, or a list of its items) under
    `torch.no_grad()` with the module in eval(), `general.save_for_freemask` on, `general.save_dir = out_dir` and
    `general.freemask_format = fmt`; `overrides` ("general.filter_out_instances=true", ...) are applied to a copy of
    `cfg` first.  The module's mode and config are restored afterwards.  A scene that `eval_step` skips (returns None)
    or for which the reader finds no usable pseudo mask is counted and named, not fatal.
    -> {"scenes": exported, "skipped": [names], "masks_per_scene": {name: K}, "bytes_written": bytes of the files}."""
    from ..datasets.utils import FreeMaskVoxelizeCollate

    if fmt not in _SUFFIXES:
        raise ValueError(f"export_round: fmt must be 'npy', 'bits' or 'both', not {fmt!r}")
    run_cfg = apply_overrides(copy.deepcopy(cfg), list(overrides))
    run_cfg.general.save_for_freemask, run_cfg.general.save_dir = True, os.fspath(out_dir)
    run_cfg.general.freemask_format = fmt
    collate = FreeMaskVoxelizeCollate(ignore_label=255, voxel_size=run_cfg.data.voxel_size, mode="validation",
                                      device=str(device))
    report = {"scenes": 0, "skipped": [], "masks_per_scene": {}, "bytes_written": 0}
    was_training, old_cfg = module.training, module.config
    module.eval()
    module.config = run_cfg
    try:
        with torch.no_grad():
            for i in range(len(scenes)):
                try:
                    item = scenes[i]
                except LookupError:                    # the reader: no usable pseudo mask in this scene
                    report["skipped"].append(export_name(scenes, i, (None,) * 4) or f"#{i}")
                    continue
                name = export_name(scenes, i, item)
                data, target, _ = collate([item])
                res = module.eval_step((data, target, [name]), i)
                if res is None:
                    report["skipped"].append(name)
                    continue
                report["scenes"] += 1
                report["masks_per_scene"][name] = int(res["instances"][0]["pred_masks"].shape[1])
                for suffix in _SUFFIXES[fmt]:
                    report["bytes_written"] += os.path.getsize(os.path.join(out_dir, "freemasks", name + suffix))
    finally:
        module.config = old_cfg
        module.train(was_training)
    return report
