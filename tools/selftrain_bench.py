"""A/B of the two self-training file formats on one synthetic scene (240 k points, 100 planted instances):

  (a) export: `save_for_freemask` fmt="npy" (bool [N,100]: device -> host -> disk) against fmt="bits" (u64 bit rows
      packed on the device), wall time per call and bytes on disk;
  (b) reader: `FreeMaskSceneReader.__getitem__` (validation mode, device_tables=True, load_self_train_data=True) over a
      directory with the bool table against one with the bit rows: the merge of the previous round's masks plus the
      device mask table, for an export on the scene's own cloud (the pipeline's case) and on a shuffled, jittered
      cloud (1-NN transfer).

One process; every variant is warmed up, then the variants alternate (A/B/A/B ...); every timed call ends in a device
synchronise.  The two reader variants must return the same table, or the tool fails.  Writes the lines to --out
(default profiles/selftrain_round.txt) and prints one JSON line.

    python tools/selftrain_bench.py [--points 240000] [--masks 100] [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_scene(n, k_export, k_own=20, seed=0):
    """[N,12] points on a 5 cm floor grid with 8 layers, `k_own` soft pseudo masks and `k_export` exported instances:
    discs of random radius around random points, so that instances overlap each other and the pseudo masks."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n / 8)))
    idx = np.arange(n)
    xyz = np.stack([(idx // 8) % side, (idx // 8) // side, idx % 8], 1) * 0.05
    pts = np.hstack([xyz, rng.uniform(0, 255, (n, 3)), rng.standard_normal((n, 3)), (idx // 50)[:, None],
                     np.zeros((n, 2))]).astype(np.float32)

    def discs(k, r_lo, r_hi):
        c = xyz[rng.integers(0, n, k), :2]
        r = rng.uniform(r_lo, r_hi, k) * side * 0.05
        return np.stack([np.hypot(xyz[:, 0] - c[j, 0], xyz[:, 1] - c[j, 1]) < r[j] for j in range(k)], 1)

    own = discs(k_own, 0.03, 0.12)
    soft = (own * rng.uniform(0.55, 1.0, (n, k_own))).astype(np.float32)
    return pts, soft, discs(k_export, 0.02, 0.15)


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0), out


def alternate(variants, repeats, dev):
    """variants {name: fn}: one warm-up of each, then `repeats` rounds in which every variant runs once, in order.
    -> {name: [ms, ...]}, {name: last result}."""
    last = {}
    for name, fn in variants.items():
        last[name] = timed(fn, dev)[1]
    ms = {name: [] for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            t, last[name] = timed(fn, dev)
            ms[name].append(t)
    return ms, last


def dir_bytes(d):
    return {f: os.path.getsize(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=240_000)
    ap.add_argument("--masks", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selftrain_round.txt"))
    a = ap.parse_args()

    from unscene3d_amd import _lib
    from unscene3d_amd.datasets.freemask import FreeMaskSceneReader
    from unscene3d_amd.trainer.postprocess import save_for_freemask

    _lib.require_device()
    dev = torch.device("cuda", 0)
    pts, soft, exported = make_scene(a.points, a.masks)
    n = pts.shape[0]
    lines = [f"selftrain_bench: {n} points, {a.masks} exported instances, {soft.shape[1]} pseudo masks, "
             f"{a.repeats} alternating repeats after one warm-up each; wall ms per call, every call ends in a device "
             f"synchronise; library: {_lib.lib.usc_build_info().decode()}"]
    result = {"points": n, "masks": a.masks, "repeats": a.repeats}
    with tempfile.TemporaryDirectory() as tmp:
        scene_dir = os.path.join(tmp, "train")
        os.makedirs(scene_dir)
        np.save(os.path.join(scene_dir, "0000_00.npy"), pts)
        np.save(os.path.join(scene_dir, "0000_00_freemasks.npy"), soft)
        entry = {"filepath": os.path.join(scene_dir, "0000_00.npy"), "raw_filepath": "raw/scene0000_00/mesh.ply"}

        # (a) the export: the predicted masks are a device bool tensor, as eval_step hands them over
        pred = torch.from_numpy(exported).to(dev)
        coords = pts[:, :3]
        dirs = {fmt: os.path.join(tmp, f"same_{fmt}") for fmt in ("npy", "bits")}
        ms, _ = alternate({fmt: (lambda fmt=fmt: save_for_freemask(dirs[fmt], "scene0000_00", coords, pred, fmt))
                           for fmt in ("npy", "bits")}, a.repeats, dev)
        sizes = {fmt: dir_bytes(os.path.join(dirs[fmt], "freemasks")) for fmt in dirs}
        for fmt in ("npy", "bits"):
            mask_file = [f for f in sizes[fmt] if "_masks" in f][0]
            lines.append(f"(a) save_for_freemask fmt={fmt:4s}: median {statistics.median(ms[fmt]):8.2f} ms  "
                         f"(min {min(ms[fmt]):.2f}, max {max(ms[fmt]):.2f})  {mask_file} {sizes[fmt][mask_file]} bytes, "
                         f"cloud {sizes[fmt]['scene0000_00_cloud.npy']} bytes")
            result[f"export_{fmt}_ms"] = statistics.median(ms[fmt])
            result[f"export_{fmt}_mask_bytes"] = sizes[fmt][mask_file]

        # (b) the reader, on the scene's own cloud and on a shuffled, jittered one
        rng = np.random.default_rng(1)
        perm = rng.permutation(n)
        jit = (coords[perm] + rng.uniform(-1e-3, 1e-3, (n, 3))).astype(np.float32)
        for fmt in ("npy", "bits"):
            dirs[f"knn_{fmt}"] = os.path.join(tmp, f"knn_{fmt}")
            save_for_freemask(dirs[f"knn_{fmt}"], "scene0000_00", jit, pred[torch.from_numpy(perm).to(dev)], fmt)
        for case, keys in (("same cloud", ("npy", "bits")), ("1-NN transfer", ("knn_npy", "knn_bits"))):
            readers = {k: FreeMaskSceneReader([entry], add_normals=False, add_raw_coordinates=True, device=str(dev),
                                              device_tables=True, load_self_train_data=True,
                                              self_train_data_dir=dirs[k], num_self_train_data=5) for k in keys}
            ms, last = alternate({k: (lambda k=k: readers[k][0]) for k in keys}, a.repeats, dev)
            t_npy, t_bits = last[keys[0]][2], last[keys[1]][2]
            if t_npy.shape != t_bits.shape or not torch.equal(t_npy, t_bits):
                raise SystemExit(f"selftrain_bench: the two readers disagree ({case})")
            for k in keys:
                fmt = k.split("_")[-1]
                lines.append(f"(b) reader item, {case:13s}, {fmt:4s}: median {statistics.median(ms[k]):8.2f} ms  "
                             f"(min {min(ms[k]):.2f}, max {max(ms[k]):.2f})  table {tuple(t_npy.shape)} (equal in both)")
                result[f"reader_{k if k.startswith('knn') else 'same_' + k}_ms"] = statistics.median(ms[k])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), file=sys.stderr)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
