"""Export a trained round's instances for the next self-training round and print one JSON line.

    python tools/export_round.py --data-dir DATA --checkpoint RUN/last.ckpt --out SELF_TRAIN
                                 [--split train|validation] [--format npy|bits|both] [--set key=value ...]

Every scene of DATA/{split}_database.yaml (the dataset tools/dataset_from_scans.py wrote) goes through
`InstanceSegmentation.eval_step` with `general.save_for_freemask` (`unscene3d_amd.trainer.rounds.export_round`), with
the weights of a `TrainLoop` checkpoint (tools/train.py --out RUN).  SELF_TRAIN/freemasks/ then holds, per scene,
`scene{id}_cloud.npy` and `scene{id}_masks.npy` (--format npy, the reference's bool table), `scene{id}_masks_bits.npy`
(--format bits: u64 bit rows, 1/8 of the bytes, merged by the reader on the device) or both: the directory
`tools/train.py --data-dir DATA --self-train-dir SELF_TRAIN` reads.

The model is built as tools/train.py --data-dir builds it (general.num_targets=3, loss.device_max_targets=128); --set
takes `a.b=value` overrides of `default_config()`, e.g. the reference's export recipe
`--set general.filter_out_instances=true general.scores_threshold=0.1 general.topk_per_image=100`.  With
`general.separate_instances=true` (and filter_out_instances) the reader re-segments every scene's mesh, or reads the
connectivity file tools/dataset_from_scans.py --write-connectivity stored, and every kept instance is exported as its
connected parts on that segmentation."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data-dir", required=True, metavar="DATA")
    ap.add_argument("--checkpoint", required=True, metavar="CKPT")
    ap.add_argument("--out", required=True, metavar="SELF_TRAIN")
    ap.add_argument("--split", default="train", choices=("train", "validation"))
    ap.add_argument("--format", default="npy", choices=("npy", "bits", "both"), dest="fmt")
    ap.add_argument("--set", nargs="*", default=[], metavar="key=value", dest="overrides")
    a = ap.parse_args()

    from unscene3d_amd.config import apply_overrides, default_config
    from unscene3d_amd.datasets.freemask import FreeMaskSceneReader, entries_from_database, load_color_mean_std
    from unscene3d_amd.trainer import InstanceSegmentation
    from unscene3d_amd.trainer.rounds import export_round, load_round_weights

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = apply_overrides(default_config(), ["general.num_targets=3", "loss.device_max_targets=128"] + list(a.overrides))
    module = InstanceSegmentation(cfg).to(dev)
    state = load_round_weights(module, a.checkpoint)
    stats = load_color_mean_std(os.path.join(a.data_dir, "color_mean_std.yaml"))
    entries = entries_from_database(os.path.join(a.data_dir, f"{a.split}_database.yaml"))
    scenes = FreeMaskSceneReader(entries, mode="validation", color_mean_std=stats, add_normals=False,
                                 add_raw_coordinates=True, device=str(dev), device_tables=True,
                                 resegment_mesh=bool(cfg.data.resegment_mesh),
                                 segment_min_vert_num=cfg.data.segment_min_vert_num)
    report = export_round(module, cfg, scenes, a.out, fmt=a.fmt, device=dev)
    torch.cuda.synchronize()
    from unscene3d_amd import _lib
    report.update({"split": a.split, "format": a.fmt, "out": a.out, "checkpoint_step": state.get("global_step"),
                   "library": _lib.lib.usc_build_info().decode()})
    print(json.dumps(report, default=float))


if __name__ == "__main__":
    main()
