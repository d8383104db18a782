#!/usr/bin/env python
"""Target building of the supervised collate (`datasets.utils.get_instance_masks`, csrc/targets.hip) on one synthetic
labelled scene (`make_scene` + `make_label_table`, --voxels 150 000, --parts 3: about 60 instances), for
    train        the voxel table with segments (labels, masks, segment_mask)
    validation   train + `target_full` from the full-resolution table
each as
    loop         the reference's per-instance loop (datasets/utils.py:529-613) written with torch operators on the device
                 — the yardstick, kept in this tool and not in the package: per instance a handful of launches and host
                 reads of tensor values
    kernel       the package's path: torch.unique + three launches + one read of T per table
The two variants alternate inside every round of ONE process (--rounds rounds of --reps back-to-back calls after
--warmup rounds); a round's time is a HIP-event span over its calls, so the host time the device waits for is inside.
Reported per variant: median, min and max of the per-call time over the rounds, and kernel / loop of the medians.
The tool asserts that both variants give identical targets.  Prints one JSON line.

    python tools/collate_bench.py [--voxels 150000] [--parts 3] [--rounds 10] [--reps 3] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unscene3d_amd import MinkowskiEngine as ME  # noqa: E402
from unscene3d_amd.datasets.utils import get_instance_masks  # noqa: E402
from unscene3d_amd.synthetic import make_label_table, make_scene  # noqa: E402

FILTER, OFFSET = [0, 1], 2


def loop_instance_masks(list_labels, list_segments=None, filter_out_classes=(), label_offset=0):
    """The reference's loop over instances, operator for operator, on device tensors."""
    target = []
    for batch_id in range(len(list_labels)):
        label_ids, masks, segment_masks = [], [], []
        labels = list_labels[batch_id]
        for instance_id in labels[:, 1].unique():
            if instance_id == -1:
                continue
            tmp = labels[labels[:, 1] == instance_id]
            label_id = tmp[0, 0]
            if label_id in filter_out_classes:
                continue
            label_ids.append(label_id)
            masks.append(labels[:, 1] == instance_id)
            if list_segments:
                segment_mask = torch.zeros(list_segments[batch_id].shape[0], device=labels.device).bool()
                segment_mask[labels[labels[:, 1] == instance_id][:, 2].unique()] = True
                segment_masks.append(segment_mask)
        if len(label_ids) == 0:
            return []
        entry = {"labels": torch.clamp(torch.stack(label_ids) - label_offset, min=0), "masks": torch.stack(masks)}
        if list_segments:
            entry["segment_mask"] = torch.stack(segment_masks)
        target.append(entry)
    return target


def measure(variants, rounds, reps, warmup):
    times = {k: [] for k in variants}
    for r in range(warmup + rounds):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b) / reps)
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                "max_ms": round(float(np.max(v)), 4)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=150_000)
    ap.add_argument("--parts", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("collate_bench: no HIP device — nothing is measured without one")
    dev = torch.device("cuda:0")
    sc = make_scene(a.seed, a.voxels)
    full = torch.from_numpy(make_label_table(sc, a.seed, parts=a.parts)).to(dev, torch.int64)
    _, unique_map, _ = ME.utils.sparse_quantize(torch.from_numpy(sc["xyz"]).to(dev), quantization_size=0.02,
                                                return_index=True, return_inverse=True, device=str(dev))
    table = full[unique_map].contiguous()
    uniq, inv = torch.unique(table[:, 2], return_inverse=True)           # what voxelize does in front of the call
    table[:, 2] = inv
    seg2label = torch.zeros((uniq.shape[0], 2), dtype=torch.int64, device=dev)

    def train(fn):
        return lambda: fn([table], list_segments=[seg2label], filter_out_classes=FILTER, label_offset=OFFSET)

    def validation(fn):
        return lambda: (train(fn)(), fn([full], filter_out_classes=FILTER, label_offset=OFFSET))

    def kernel(tables, **kw):
        return get_instance_masks(tables, "instance_segmentation", **kw)

    for mode in (train, validation):                                     # identical targets first
        got, want = mode(kernel)(), mode(loop_instance_masks)()
        got, want = (got, want) if mode is validation else ((got,), (want,))
        for g, w in zip(got, want):
            assert len(g) == len(w) == 1 and all(torch.equal(g[0][k], w[0][k]) for k in w[0]), "variants differ"
    n_targets = int(kernel([table], filter_out_classes=FILTER, label_offset=OFFSET)[0]["labels"].shape[0])
    out = {"voxels": int(table.shape[0]), "points": int(full.shape[0]), "segments": int(uniq.shape[0]),
           "instance_ids": int(torch.unique(table[:, 1]).shape[0]), "targets": n_targets, "rounds": a.rounds,
           "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for name, mode in (("train", train), ("validation", validation)):
        res = measure({"loop": mode(loop_instance_masks), "kernel": mode(kernel)}, a.rounds, a.reps, a.warmup)
        res["kernel_over_loop"] = round(res["kernel"]["median_ms"] / res["loop"]["median_ms"], 4)
        out[name] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
