#!/usr/bin/env python
"""Validation-metric cost: the device overlap histogram (ops.mask_gt_overlap) of one 150 k-point scene with K = 100
predicted masks and G = 30 GT instances, in slot-sorted and in random point order, and with G = 1 000; plus the host
matching (InstanceAPEvaluator.compute) of a 312-scene split (ScanNet's validation set) built from that scene's table.

Kernel times are HIP-event medians over --reps back-to-back calls (one call per scene in real use).  Prints one JSON
line.

    python tools/eval_bench.py [--reps 50] [--scenes 312]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unscene3d_amd import ops  # noqa: E402
from unscene3d_amd.evaluation import FREEMASK, InstanceAPEvaluator, SceneGT  # noqa: E402


def make_scene(rng, n=150_000, k=100, g=30, sort=False):
    """GT ids (g instances of label 1, the rest void) and K masks: noisy copies of GT instances plus random ones."""
    sizes = rng.integers(max(1, n // (4 * g)), max(2, 3 * n // (4 * g)), g)
    sizes = np.minimum(sizes, (n - 1) // g)
    ids = np.zeros(n, np.int64)
    perm = rng.permutation(n)
    pos = 0
    for i, sz in enumerate(sizes):
        ids[perm[pos:pos + sz]] = 1000 + i + 1
        pos += sz
    if sort:
        ids = np.sort(ids)
    masks = np.zeros((n, k), bool)
    for j in range(k):
        if j % 3 != 2:
            src = np.nonzero(ids == 1000 + 1 + (j % g))[0]
            masks[src[rng.random(src.size) < 0.8], j] = True
        masks[rng.choice(n, int(rng.integers(100, 3000)), replace=False), j] = True
    scores = rng.random(k).astype(np.float32)
    classes = (rng.random(k) < 0.9).astype(np.int64)
    return ids, masks, scores, classes


def time_kernel(masks_dev, slot_dev, nslots, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(3):
        ops.mask_gt_overlap(masks_dev, slot_dev, nslots)
    for a, b in ev:
        a.record()
        ops.mask_gt_overlap(masks_dev, slot_dev, nslots)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) * 1000.0 for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--scenes", type=int, default=312)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    out = {"n_points": 150_000, "k": 100}
    tables = {}
    for tag, g, sort in (("g30_sorted", 30, True), ("g30_random", 30, False), ("g1000_random", 1000, False)):
        ids, masks, scores, classes = make_scene(rng, g=g, sort=sort)
        sg = SceneGT(ids, FREEMASK)
        m, s = torch.from_numpy(masks).to(dev), torch.from_numpy(sg.slot).to(dev)
        out[f"kernel_us_{tag}"] = round(time_kernel(m, s, sg.nslots, a.reps), 2)
        tables[tag] = (ids, m, scores, classes)
    out["kernel_ms_312_scenes_random"] = round(out["kernel_us_g30_random"] * 312 / 1000.0, 3)

    # host matching of a whole split from device tables (add_scene issues the histogram; compute reads back once)
    ids, m, scores, classes = tables["g30_random"]
    ev = InstanceAPEvaluator(FREEMASK)
    inst = {"pred_masks": m, "pred_scores": scores, "pred_classes": classes}
    for i in range(a.scenes):
        ev.add_scene(f"scene{i:04d}_00", inst, gt_ids=ids)          # GT prepared once per scene name
    torch.cuda.synchronize()
    ev.reset()
    t0 = time.perf_counter()
    for i in range(a.scenes):
        ev.add_scene(f"scene{i:04d}_00", inst)
    t1 = time.perf_counter()
    r = ev.compute()
    t2 = time.perf_counter()
    out["scenes"] = a.scenes
    out["add_scene_s_total"] = round(t1 - t0, 4)
    out["compute_s_total"] = round(t2 - t1, 4)
    out["split_s_total"] = round(t2 - t0, 4)
    out["ap50"] = float(r["avg_ap"]["all_ap_50%"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
