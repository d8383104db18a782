#!/usr/bin/env python
"""Per-scene time of `FreeMaskSceneReader.__getitem__` (train mode) with the mask tables built on the host (numpy, the
default) and on the device (`device_tables=True`, csrc/dataset.hip), on generated files of real size.

    python tools/reader_bench.py [--points 200000] [--masks 20 40] [--scenes 20] [--warmup 3] [--out profiles/reader_tables.json]
                                 [--step-ms MS]

For every K of --masks one scene file of --points points is generated ([N,12] table + [N,K] soft masks: K compact blobs
that pass the extent filter, soft values on both sides of the threshold) and read --scenes times after --warmup reads
per path, the two paths alternated A/B read by read; every read ends in a device synchronisation, so the time covers
the uploads and the kernels.  The reader is the one tools/train.py --data-dir builds (shipped augmentations,
add_normals=False, add_raw_coordinates=True).  --step-ms: the training step time of the same session
(`tools/train.py --synthetic`), written beside the numbers."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_scene_files(d, n, k, seed):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(0, 8, n), rng.uniform(0, 6, n), rng.uniform(0, 2.5, n)], 1)
    points = np.zeros((n, 12), np.float32)
    points[:, :3] = xyz
    points[:, 3:6] = rng.integers(0, 256, (n, 3))
    nrm = rng.normal(0, 1, (n, 3))
    points[:, 6:9] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    points[:, 9] = np.floor(xyz[:, 0] * 4) * 64 + np.floor(xyz[:, 1] * 4)            # ~800 segments
    centres = np.stack([rng.uniform(1, 7, k), rng.uniform(1, 5, k)], 1)
    dist = np.linalg.norm(xyz[:, None, :2] - centres[None], axis=-1)
    soft = np.clip(1.0 - dist / rng.uniform(0.5, 1.5, k), 0, 1).astype(np.float32)       # > 0.5 within half the radius
    path = os.path.join(d, "train", "0000_00.npy")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.save(path, points)
    np.save(path.replace(".npy", "_freemasks.npy"), soft)
    return {"filepath": path, "raw_filepath": "scans/scene0000_00/scene0000_00_vh_clean_2.ply"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--masks", type=int, nargs="+", default=[20, 40])
    ap.add_argument("--scenes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from unscene3d_amd import _lib
    from unscene3d_amd.datasets.augment import ColorAugmentations, VolumeAugmentations
    from unscene3d_amd.datasets.freemask import FreeMaskSceneReader

    dev = torch.device("cuda", torch.cuda.current_device())
    result = {"points": a.points, "scenes": a.scenes, "warmup": a.warmup, "train_step_ms": a.step_ms, "cases": [],
              "library": _lib.lib.usc_build_info().decode()}
    for k in a.masks:
        with tempfile.TemporaryDirectory() as d:
            entry = make_scene_files(d, a.points, k, seed=k)
            readers = {name: FreeMaskSceneReader([entry], mode="train", volume_augmentations=VolumeAugmentations(),
                                                 image_augmentations=ColorAugmentations(), add_normals=False,
                                                 add_raw_coordinates=True, device=str(dev), device_tables=flag)
                       for name, flag in (("host", False), ("device", True))}
            times = {name: [] for name in readers}
            kept = {}
            for i in range(a.warmup + a.scenes):
                for name, reader in readers.items():
                    np.random.seed(i)
                    random.seed(i)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    item = reader[0]
                    torch.cuda.synchronize()
                    if i >= a.warmup:
                        times[name].append(1e3 * (time.perf_counter() - t0))
                    kept[name] = item[2]
            same = bool(np.array_equal(kept["host"], kept["device"].cpu().numpy()))
            case = {"masks": k, "masks_kept": int(kept["host"].shape[1] - 2), "tables_equal": same}
            for name, t in times.items():
                case[f"{name}_ms_p10_p50_p90"] = [round(float(np.percentile(t, q)), 3) for q in (10, 50, 90)]
                case[f"{name}_ms_mean"] = round(float(np.mean(t)), 3)
            case["speedup_p50"] = round(case["host_ms_p10_p50_p90"][1] / case["device_ms_p10_p50_p90"][1], 3)
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
