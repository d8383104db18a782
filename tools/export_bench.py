"""Cost of the export post-processing at scene size: 150 k voxels, 240 k full-resolution
points, 100 queries, freemask settings (filter on, no DBSCAN) — device path vs the same host logic on torch CPU ops.

    python tools/export_bench.py [--reps 10]
    python tools/export_bench.py --dbscan [--pairs 5]

--dbscan: the eval-time DBSCAN split alone (general.use_dbscan, eps 0.95, min_points 1) on a room of about 150 k
voxels with 150 planted query masks (the floor, four walls, boxes, masks made of two or three separated boxes, wall
patches, empty queries): the per-query route `postprocess.dbscan_split` (A) against the batched one
`dbscan_split_batched` (B) in one process, A/B/A/B after a warm-up of each, time per scene with its spread.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace as NS

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unscene3d_amd import ops  # noqa: E402
from unscene3d_amd.trainer import postprocess as PP  # noqa: E402


def scene(seed, n_low=150_000, n_full=240_000, S=2500, Q=100):
    rng = np.random.default_rng(seed)
    p2s = rng.integers(0, S, n_low)
    inverse = np.concatenate([np.arange(n_low), rng.integers(0, n_low, n_full - n_low)])
    seg_full = p2s[inverse].copy()
    flip = rng.random(n_full) < 0.04
    seg_full[flip] = rng.integers(0, S, int(flip.sum()))
    obj = rng.integers(0, 40, S)
    masks = rng.normal(-4, 1, (S, Q)).astype(np.float32)
    for q in range(60):
        masks[:, q] = np.where(obj == q % 40, 4.0, -4.0)
    logits = rng.normal(0, 1, (1, Q, 3)).astype(np.float32)
    logits[0, :60, 1] += 3
    return p2s, inverse, seg_full, masks, logits


def run(dev, data, general):
    p2s, inverse, seg_full, masks, logits = data
    output = {"aux_outputs": [], "pred_logits": torch.from_numpy(logits).to(dev),
              "pred_masks": [torch.from_numpy(masks).to(dev)]}
    low = [{"point2segment": torch.from_numpy(p2s).to(dev)}]
    full = [{"point2segment": torch.from_numpy(seg_full).to(dev)}]
    inv = [torch.from_numpy(inverse).to(dev)]
    return lambda: PP.export_instances(output, low, full, inv, None, general, num_classes=3)


def dbscan_scene(seed=0, Q=150):
    """-> xyz f32[N,3] (2 cm voxels of a 4 x 4 x 2 m room with 64 boxes on the floor), mask logits f32[N,Q]."""
    rng = np.random.default_rng(seed)
    side, height, box, pitch = 200, 100, 10, 24
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    parts, tags = [np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3)], [np.zeros(side * side, np.int64)]
    u, v = np.meshgrid(np.arange(side), np.arange(1, height + 1), indexing="ij")
    u, v = u.ravel(), v.ravel()
    for w, wall in enumerate((np.stack([u, 0 * u, v], 1), np.stack([u, 0 * u + side - 1, v], 1),
                              np.stack([0 * u, u, v], 1), np.stack([0 * u + side - 1, u, v], 1))):
        parts.append(wall)
        tags.append(np.full(len(wall), 1 + w))
    a = np.arange(box)
    cube = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    shell = cube[((cube == 0) | (cube == box - 1)).any(1)]
    for b in range(64):
        parts.append(shell + np.array([8 + pitch * (b // 8), 8 + pitch * (b % 8), 1]))
        tags.append(np.full(len(shell), 5 + b))
    vox, first = np.unique(np.concatenate(parts), axis=0, return_index=True)
    tag = np.concatenate(tags)[first]
    perm = rng.permutation(len(vox))
    vox, tag = vox[perm], tag[perm]
    on = np.zeros((len(vox), Q), bool)
    for q in range(5):                                          # the floor and the four walls
        on[:, q] = tag == q
    for q in range(5, 45):                                      # one box each
        on[:, q] = tag == q
    far = lambda b, c: max(abs(b // 8 - c // 8), abs(b % 8 - c % 8)) >= 3      # gap >= 62 voxels = 1.24 m > eps
    for q in range(45, 70):                                     # two (45-59) or three (60-69) separated boxes
        boxes = [int(rng.integers(0, 64))]
        while len(boxes) < (2 if q < 60 else 3):
            c = int(rng.integers(0, 64))
            if all(far(b, c) for b in boxes):
                boxes.append(c)
        on[:, q] = np.isin(tag, 5 + np.array(boxes))
    for q in range(70, 130):                                    # 0.6 m patches of a wall
        w = 1 + q % 4
        c = vox[rng.choice(np.flatnonzero(tag == w))]
        on[:, q] = (tag == w) & (np.abs(vox - c) <= 15).all(1)
    mag = rng.uniform(2.0, 6.0, on.shape).astype(np.float32)   # queries 130-149 stay empty
    return (vox * 0.02).astype(np.float32), np.where(on, mag, -mag).astype(np.float32)


def dbscan_ab(pairs):
    dev = torch.device("cuda:0")
    xyz, logits = dbscan_scene()
    xyz, masks = torch.from_numpy(xyz).to(dev), torch.from_numpy(logits).to(dev)
    cls = torch.randn(masks.shape[1], 3, device=dev)
    routes = {"per_query": lambda: PP.dbscan_split(masks, cls, xyz, 0.95),
              "batched": lambda: PP.dbscan_split_batched(masks, cls, xyz, 0.95, 1)}
    out = {k: fn() for k, fn in routes.items()}                 # warm-up of each route
    torch.cuda.synchronize()
    equal = all(torch.equal(a, b) for a, b in zip(out["per_query"], out["batched"]))
    ms = {k: [] for k in routes}
    for _ in range(pairs):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {"voxels": int(masks.shape[0]), "queries": int(masks.shape[1]), "columns": int(out["batched"][0].shape[1]),
           "largest_mask": int((masks > 0).sum(0).max()), "eps": 0.95, "min_points": 1, "pairs": pairs,
           "results_equal": equal}
    for k, v in ms.items():
        res[k + "_ms_per_scene"] = {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dbscan", action="store_true", help="A/B of the per-query and the batched DBSCAN split")
    ap.add_argument("--pairs", type=int, default=5, help="--dbscan: A/B pairs after the warm-up (at least 3)")
    a = ap.parse_args()
    if a.dbscan:
        dbscan_ab(max(3, a.pairs))
        return
    general = NS(use_dbscan=False, dbscan_eps=0.95, topk_per_image=100, filter_out_instances=True, scores_threshold=0.1,
                 iou_threshold=0.66)
    data = scene(0)
    fn = run(torch.device("cuda:0"), data, general)
    res = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        fn()
    torch.cuda.synchronize()
    gpu_ms = (time.perf_counter() - t0) / a.reps * 1e3

    # the same host logic on torch CPU ops (what the reference's CPU path costs)
    real = {k: getattr(ops, k) for k in ("gather_rows", "segment_csr", "segment_mean")}
    ops.gather_rows = lambda src, idx: src[idx]
    ops.segment_csr = lambda seg, S: ops.SegmentCSR(seg, None, None, S)

    def segment_mean(src, csr):
        out = torch.zeros((csr.S, src.shape[1])).index_add_(0, csr.seg, src)
        cnt = torch.zeros(csr.S).index_add_(0, csr.seg, torch.ones(src.shape[0]))
        return out / cnt.clamp(min=1)[:, None]

    ops.segment_mean = segment_mean
    cfn = run(torch.device("cpu"), data, general)
    t0 = time.perf_counter()
    cres = cfn()
    cpu_ms = (time.perf_counter() - t0) * 1e3
    for k, v in real.items():
        setattr(ops, k, v)
    same = bool(np.array_equal(res[0]["pred_masks"].cpu().numpy(), cres[0]["pred_masks"].numpy()))
    print(json.dumps({"voxels": 150_000, "points": 240_000, "queries": 100, "kept": int(res[0]["pred_masks"].shape[1]),
                      "device_ms_per_scene": gpu_ms, "torch_cpu_ms_per_scene": cpu_ms,
                      "cpu_threads": torch.get_num_threads(), "masks_equal": same}))


if __name__ == "__main__":
    main()
